// vrl.hip.h — the virtual ray lights' two kernels (src/integrators/explicit/vol_primitives.rs:201-253, 705-790, `VRL` arm).  Per camera sample the reference
// gathers the surface beams through the beam tree (no draws), then walks every VRL in storing order: one roulette draw each, and for a VRL that survives two
// more draws (t_cam, t_vrl) and one visibility ray.  A sample so takes 2 + n_vrl + 2 A draws, A the VRLs that survived in it, and where a later sample of the
// block starts in the block's stream depends on every A before it.
//
// k_vrl_chain, the chain pass.  Which VRLs survive depends on the block's stream and the rr table alone, not on the scene: one lane per owned block walks the
// block's stream pixel by pixel (ix outer, iy inner, spp samples each; 2 draws, then per VRL 1 draw and 2 more if rr >= u) and writes the draw index at which
// every pixel starts ([owned block][256] u32) and the block's total.  No scene data, one instantiation (vrl_lds.hip holds it).
//
// k_vrl_gather<LDS_SCENE>.  pplane_gather's frame (pplane.hip.h): workgroup = owned block, lane = pixel c = ix * bh + iy.  The lane enters the stream at its
// pixel's chained start, walks the beam tree with BeamLeaf (beam.hip.h) unchanged and then the VRLs, into the same cs.  VRL: 3 float4 = o, length | d, rr |
// radiance, 0 (rr = ((channel_max(radiance) / avg) * 0.01).min(1.0), computed on the host).
//
// The VRL loop.  The roulette passes about 1 % of the VRLs per lane, so evaluating a VRL where it is accepted would run the visibility ray and the two exp
// triples at one or two live lanes in every second iteration.  A lane instead takes its draws in stream order and queues (vrl, t_cam, t_vrl) in a four-entry
// FIFO held in registers (q0 is the oldest; no indexed access, so no private segment); the wave evaluates the oldest entry of every lane that has one once
// kVrlWaveFill lanes have one pending or a queue is full, and drains the queues at the end of the sample.  A lane's entries are evaluated oldest first, which
// is VRL order, and the beams were added before: cs sums in the reference's order.
//
// contribute_vrl statement by statement: p_vrl = o + d * t_vrl, p_cam = ray.o + ray.d * t_cam, visible(p_cam, p_vrl) — this argument order —, dist = |p_vrl -
// p_cam|, radiance * (sigma_s / 4 PI) * (sigma_s / 4 PI) * transmittance(t_cam) * transmittance(dist), * inv_pdf / (dist * dist), / rr, * norm_photon, left
// to right with Color's guards (a non-finite factor and a zero or non-finite divisor give black).  dist == 0: the reference asserts in Ray::new on the NaN
// direction; here the direction is never formed (the phase function is Isotropic) and the guarded divide by dist * dist = 0 gives black.
//
// Statistics: k_pplane_gather's eight rows — nodes entered, beams accepted, VRLs that passed the roulette, of those visible — as a low and a high row each.
#pragma once
#include "beam.hip.h"

namespace rl {

static constexpr unsigned kVrlWaveFill = 40u;      // lanes of a wave with a pending entry that make the wave evaluate

// k_vrl_chain's body (the kernel itself is in vrl_lds.hip: it is no template, and one object holds it)
RL_DEV void vrl_chain(const RenderConst& rc, const VrlConst& vc) {
    const unsigned ob = blockIdx.x * blockDim.x + threadIdx.x;
    if (ob >= rc.n_owned) return;
    unsigned bx, by, bw, bh;
    block_geometry(rc, rc.owned_blocks[ob], &bx, &by, &bw, &bh);
    Rng rng = rng_seed(rc.block_seeds[rc.owned_blocks[ob]], rc.seed_variant);
    unsigned n = 0u;
    const unsigned n_px = bw * bh;
    for (unsigned c = 0; c < n_px; c++) {
        vc.starts[(size_t)ob * 256u + c] = n;
        for (unsigned s = 0; s < rc.spp; s++) {
            rng_next_u64(rng); rng_next_u64(rng);                          // the pixel jitter
            n += 2u;
            for (unsigned i = 0; i < vc.n_vrl; i++) {
                const float rr = vc.vrls[3u * (size_t)i + 1u].w;
                n++;
                if (rr >= rng_next_f32(rng)) { rng_next_u64(rng); rng_next_u64(rng); n += 2u; }      // t_cam, t_vrl
            }
        }
    }
    vc.totals[ob] = n;
}

// one accepted VRL of one lane: PhotonBeam::contribute_vrl with the draws already taken, then `/ rr) * norm_photon`
template <class STACK>
RL_DEV void vrl_contribute(const VrlConst& vc, unsigned idx, float t_cam, float t_vrl, V3 cam, V3 rd, float tfar, const DeviceScene& sc, const SceneRecs& recs,
                           const STACK& stack, Col& cs, unsigned long long& n_visible) {
    const float4* vr = vc.vrls + 3u * (size_t)idx;
    const float4 q0 = vr[0], q1 = vr[1];
    const V3 p_vrl = mk3(q0.x, q0.y, q0.z) + mk3(q1.x, q1.y, q1.z) * t_vrl;
    const V3 p_cam = cam + rd * t_cam;
    if (!shadow_visible(sc, recs, stack, p_cam, p_vrl)) return;
    n_visible++;
    const float4 q2 = vr[2];
    const float inv_pdf = q0.w * (tfar - kEps);                            // self.length * (ray.tfar - ray.tnear)
    const float dist = length(p_vrl - p_cam);
    const Col trans_cam = medium_transmittance(sc.medium, t_cam);
    const Col trans_vrl = medium_transmittance(sc.medium, dist);
    const Col phase = mkc(sc.medium.sigma_s[0], sc.medium.sigma_s[1], sc.medium.sigma_s[2]) * cval(div_rn(1.0f, kPi * 4.0f));      // m.sigma_s * Isotropic.eval(..), both ends
    const Col contrib = (((mkc(q2.x, q2.y, q2.z) * phase) * phase) * trans_cam) * trans_vrl;
    cs = cs + (((contrib * inv_pdf) / (dist * dist)) / q1.w) * vc.beam.norm_photon;
}

template <bool LDS_SCENE>
RL_DEV void vrl_gather(const RenderConst& rc, const DeviceScene& sc, const StackConf& stc, float4* smem, const VrlConst& vc) {
    const BeamLeaf beams{vc.beam};
    SceneRecs recs;
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x;
    const TravStackT<LDS_SCENE> stack = open_scene<LDS_SCENE>(sc, stc, smem, tid, &recs);
    const unsigned ob = blockIdx.x, c = threadIdx.x;
    unsigned bx, by, bw, bh;
    block_geometry(rc, rc.owned_blocks[ob], &bx, &by, &bw, &bh);
    const bool active = c < bw * bh;
    unsigned long long n_entered = 0, n_beam[1] = {}, n_accepted = 0, n_visible = 0;
    if (active) {
        Rng rng = rng_seed(rc.block_seeds[rc.owned_blocks[ob]], rc.seed_variant);
        rng_advance<false>(rng, vc.starts[(size_t)ob * 256u + c]);         // the pixel's chained start
        const unsigned ix = c / bh, iy = c - (c / bh) * bh;
        const V3 cam = mk3(sc.camera.position[0], sc.camera.position[1], sc.camera.position[2]);
        Col sum = czero();
        for (unsigned s = 0; s < rc.spp; s++) {
            const float u = (float)(bx + ix) + rng_next_f32(rng);         // Point2::new(ix_c + next(), iy_c + next())
            const float v = (float)(by + iy) + rng_next_f32(rng);
            const V3 rd = camera_direction(sc, u, v);
            Hit hit;
            const float tfar = trace_closest(sc, recs, stack, cam, rd, hit) ? hit.t : kF32Max;     // ray.tfar = max_dist; a miss still takes its draws
            const V3 inv_d = mk3(div_rn(1.0f, rd.x), div_rn(1.0f, rd.y), div_rn(1.0f, rd.z));
            Col cs = czero();
            unsigned i = 0u;
            while (i < vc.beam.n_nodes) {                                   // bvh_beams.gather(&ray): the surface beams
                const float4 a = vc.beam.nodes[2u * i], b = vc.beam.nodes[2u * i + 1u];
                float te;
                if (!slab(mk3(a.x, a.y, a.z), mk3(a.w, b.x, b.y), cam, inv_d, kEps, tfar, &te)) { i = __float_as_uint(b.z); continue; }
                n_entered++;
                const unsigned fc = __float_as_uint(b.w), first = fc >> 3, count = fc & 7u;
                for (unsigned k = 0; k < count; k++) beams.element(first + k, cam, rd, tfar, sc, recs, stack, cs, n_beam);
                i++;
            }
            // for vrl in vrls: the FIFO, q0 the oldest
            unsigned cnt = 0u, i0 = 0u, i1 = 0u, i2 = 0u, i3 = 0u;
            float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f, v0 = 0.0f, v1 = 0.0f, v2 = 0.0f, v3 = 0.0f;
            const float span = tfar - kEps;                                 // ray.tfar - ray.tnear
            for (unsigned k = 0; k <= vc.n_vrl; k++) {
                const bool last = k == vc.n_vrl;
                if (!last && vc.vrls[3u * (size_t)k + 1u].w >= rng_next_f32(rng)) {        // if rr >= sampler.next()
                    const float t_cam = span * rng_next_f32(rng) + kEps;
                    const float t_vrl = vc.vrls[3u * (size_t)k].w * rng_next_f32(rng);
                    n_accepted++;
                    if (cnt == 0u) { i0 = k; c0 = t_cam; v0 = t_vrl; }
                    else if (cnt == 1u) { i1 = k; c1 = t_cam; v1 = t_vrl; }
                    else if (cnt == 2u) { i2 = k; c2 = t_cam; v2 = t_vrl; }
                    else { i3 = k; c3 = t_cam; v3 = t_vrl; }
                    cnt++;
                }
                // the wave's decision: evaluate now (once), or — after the last VRL — until every queue is empty
                for (;;) {
                    const unsigned long long pending = __ballot(cnt > 0u);
                    if (pending == 0ull) break;
                    if (!last && (unsigned)__popcll(pending) < kVrlWaveFill && __ballot(cnt == 4u) == 0ull) break;
                    if (cnt > 0u) {
                        vrl_contribute(vc, i0, c0, v0, cam, rd, tfar, sc, recs, stack, cs, n_visible);
                        i0 = i1; c0 = c1; v0 = v1; i1 = i2; c1 = c2; v1 = v2; i2 = i3; c2 = c3; v2 = v3;
                        cnt--;
                    }
                    if (!last) break;
                }
            }
            sum = sum + cs;                                                 // im_block.accumulate, in sample order
        }
        const Col px = scale_unguarded(sum, rc.inv_spp);                    // im_block.scale(1 / spp)
        const size_t pix = (size_t)(by + iy) * rc.W + (bx + ix);
        rc.out[3 * pix] = px.r; rc.out[3 * pix + 1] = px.g; rc.out[3 * pix + 2] = px.b;
    }
    {
        static constexpr int rows[8] = {STAT_GATHER_NODES, STAT_GATHER_NODES_HI, STAT_PPLANE_BEAMS, STAT_PPLANE_BEAMS_HI, STAT_PPLANE_ISECT, STAT_PPLANE_ISECT_HI,
                                        STAT_PPLANE_VISIBLE, STAT_PPLANE_VISIBLE_HI};
        unsigned vals[8];
        gather_split24(n_entered, &vals[0], &vals[1]);
        gather_split24(n_beam[0], &vals[2], &vals[3]);
        gather_split24(n_accepted, &vals[4], &vals[5]);
        gather_split24(n_visible, &vals[6], &vals[7]);
        block_stats<8>(rc.partials, rows, vals);
    }
}

template <bool LDS_SCENE>
__global__ void __launch_bounds__(256) k_vrl_gather(RenderConst rc, DeviceScene sc, StackConf stc, VrlConst vc) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    vrl_gather<LDS_SCENE>(rc, sc, stc, smem, vc);
}

}  // namespace rl
