// bre.hip.h — the beam radiance estimate of IntegratorVolPrimitives (src/integrators/explicit/vol_primitives.rs:41-98, 712-790): the volume photons of a
// light pass (the records of rl_vpl_generate with RL_VPL_VOLUME: convert_photons stores what convert_vpl stores under `-v volume`) are gathered along every
// camera ray through a tree of photon spheres.  Instantiated by bre_lds.hip (scene staged in LDS) and bre_stream.hip (BVH streamed from L2 / HBM).
//
// A camera sample takes exactly 2 draws (the pixel jitter), so sample (ix, iy, s) of a block starts at draw ((ix * bh + iy) * spp + s) * 2 of the block's
// stream (ix outer, vol_primitives.rs:712-714): a lane enters its pixel's place with one rng_advance and walks the pixel's samples in order, which is also the
// order im_block.accumulate adds them in.
//
// The photon tree (host/photontree.cpp) is stored in the order BHVAccel::gather (accel.rs:545-581) visits it — node, right subtree, left subtree — with a skip
// link per node, so the walk is `i = entered ? i + 1 : skip` and keeps no stack; a leaf tests its photons in index order, and the contributions are added in
// that order (f32 sums depend on it).  Node: 2 float4 = p_min.xyz, p_max.x | p_max.yz, skip, first << 3 | count (count = 0: inner node).  Photon: 3 float4 =
// pos | radiance | d_in; the radiance is loaded for accepted photons only, d_in only by the Henyey-Greenstein instantiation.
#pragma once
#include "rngjump.h"        // rng_advance

namespace rl {

// k_bre_gather<LDS_SCENE, HG> — workgroup = one owned block, lane c = ix * bh + iy of it.  HG: the medium's phase function is Henyey-Greenstein
template <bool LDS_SCENE, bool HG>
__global__ void __launch_bounds__(256) k_bre_gather(RenderConst rc, DeviceScene sc, StackConf stc, BreConst bc) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneRecs recs;
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x;
    const TravStackT<LDS_SCENE> stack = open_scene<LDS_SCENE>(sc, stc, smem, tid, &recs);
    const unsigned ob = blockIdx.x, c = threadIdx.x;
    unsigned bx, by, bw, bh;
    block_geometry(rc, rc.owned_blocks[ob], &bx, &by, &bw, &bh);
    const bool active = c < bw * bh;
    unsigned n_samples = 0;
    unsigned long long n_entered = 0, n_gathered = 0;       // (a lane may enter more than 2^32 nodes over its samples)
    if (active) {
        Rng rng = rng_seed(rc.block_seeds[rc.owned_blocks[ob]], rc.seed_variant);
        rng_advance<false>(rng, c * rc.spp * 2u);
        const unsigned ix = c / bh, iy = c - (c / bh) * bh;
        const V3 cam = mk3(sc.camera.position[0], sc.camera.position[1], sc.camera.position[2]);
        Col sum = czero();
        for (unsigned s = 0; s < rc.spp; s++) {
            n_samples++;
            const float u = (float)(bx + ix) + rng_next_f32(rng);         // Point2::new(ix_c + next(), iy_c + next())
            const float v = (float)(by + iy) + rng_next_f32(rng);
            const V3 rd = camera_direction(sc, u, v);
            Hit hit;
            const float tfar = trace_closest(sc, recs, stack, cam, rd, hit) ? hit.t : kF32Max;     // ray.tfar = max_dist; a miss still gathers
            const V3 inv_d = mk3(div_rn(1.0f, rd.x), div_rn(1.0f, rd.y), div_rn(1.0f, rd.z));
            Col cs = czero();
            unsigned i = 0u;
            while (i < bc.n_nodes) {
                const float4 a = bc.nodes[2u * i], b = bc.nodes[2u * i + 1u];
                float te;
                if (!slab(mk3(a.x, a.y, a.z), mk3(a.w, b.x, b.y), cam, inv_d, kEps, tfar, &te)) { i = __float_as_uint(b.z); continue; }
                n_entered++;
                const unsigned fc = __float_as_uint(b.w), first = fc >> 3, count = fc & 7u;
                for (unsigned k = 0; k < count; k++) {
                    const float4* ph = bc.photons + 3u * (size_t)(first + k);
                    const float4 q0 = ph[0];
                    const V3 pos = mk3(q0.x, q0.y, q0.z);
                    const float along = dot(pos - cam, rd);                // Photon::intersection (vol_primitives.rs:63-78)
                    if (along <= 0.0f || along > tfar) continue;
                    const V3 p = cam + rd * along;
                    if (length2(pos - p) > bc.radius2) continue;
                    n_gathered++;
                    const float4 q1 = ph[1];                                // Photon::contribute (81-98), then `* norm_photon`
                    const Col trans = medium_transmittance(sc.medium, along);
                    Col phase;
                    if (HG) { const float4 q2 = ph[2]; phase = phase_eval(sc.medium, -rd, mk3(q2.x, q2.y, q2.z)); }
                    else phase = cval(div_rn(1.0f, kPi * 4.0f));
                    cs = cs + (((mkc(q1.x, q1.y, q1.z) * trans) * phase) * bc.kernel) * bc.norm_photon;
                }
                i++;
            }
            sum = sum + cs;                                                 // im_block.accumulate, in sample order
        }
        const Col px = scale_unguarded(sum, rc.inv_spp);                    // im_block.scale(1 / spp)
        const size_t pix = (size_t)(by + iy) * rc.W + (bx + ix);
        rc.out[3 * pix] = px.r; rc.out[3 * pix + 1] = px.g; rc.out[3 * pix + 2] = px.b;
    }
    {
        // block_stats sums 32-bit values over the workgroup: the two tree counters go through it as 24 low bits and the rest (rows STAT_BRE_*_HI)
        const int which[7] = {STAT_SAMPLES, STAT_EXT_RAYS, STAT_DRAWS, STAT_BRE_NODES, STAT_BRE_PHOTONS, STAT_BRE_NODES_HI, STAT_BRE_PHOTONS_HI};
        const unsigned vals[7] = {n_samples, n_samples, 2u * n_samples, (unsigned)n_entered & 0xffffffu, (unsigned)n_gathered & 0xffffffu,
                                  (unsigned)(n_entered >> 24), (unsigned)(n_gathered >> 24)};
        block_stats<7>(rc.partials, which, vals);
    }
}

template <bool LDS_SCENE>
static void launch_bre_impl(bool hg, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const BreConst& bc) {
    with_flag(hg, [&](auto H) { hipLaunchKernelGGL((k_bre_gather<LDS_SCENE, decltype(H)::value>), grid, block, lds_bytes, st, rc, ds, stc, bc); });
}

}  // namespace rl
