// pplane.hip.h — the photon planes' gather (src/integrators/explicit/vol_primitives.rs:256-373, 705-790, `Planes` arm): every camera sample walks two trees, the
// surface beams' (host/beamtree.cpp) and the planes' (host/planetree.cpp), and adds what both contribute into one colour before the sample is accumulated.  In
// f32 the sum over samples of (beams + planes) is not the sum of the two sums, so the two walks share a kernel: k_pplane_gather<LDS_SCENE>, instantiated by
// pplane_lds.hip (scene staged in LDS) and pplane_stream.hip (BVH streamed from L2 / HBM).
//
// The frame is beam_gather's (gather.hip.h): a workgroup per owned block, lane c = ix * bh + iy, entry at draw c * spp * 2 of the block's stream, tfar = the
// closest hit or f32::MAX, a stackless walk per tree.  beam_gather walks one tree per sample and is left as it is; its two-tree form is pplane_gather below.
// The beam tree's element is BeamLeaf (beam.hip.h), unchanged.  The plane tree's element is PPlaneLeaf: plane_intersect (plane.hip.h) with (kEps, tfar), one
// visibility ray visible(p0, p_its) — the reference's argument order, the opposite of plane-single's —, then
// radiance * 1/(4 PI) * sigma_s * sigma_s * transmittance(t_cam) * (1 / |d0 . (d1 x -rd)|) * norm_photon, left to right.  The phase function is Isotropic
// whatever the medium's is (:410).  Plane: 4 float4 = o, length0 | d0, length1 | d1, 0 | radiance, 0; the radiance is loaded for visible planes only.
//
// Statistics.  Four 64-bit walk counters — nodes entered in both trees, beams accepted, planes intersected, of those visible — go through block_stats as a low
// and a high row each (launch.h: gather_split24): all STAT_COUNT = 8 rows.  The samples have no row of their own: a lane takes exactly spp samples per owned
// pixel, so the host sets camera_samples = owned pixels * spp (GatherKind::derive_samples).
#pragma once
#include "beam.hip.h"
#include "plane.hip.h"

namespace rl {

struct PPlaneLeaf {
    PPlaneConst c;
    template <class STACK>
    RL_DEV void element(unsigned idx, V3 cam, V3 rd, float tfar, const DeviceScene& sc, const SceneRecs& recs, const STACK& stack, Col& cs, unsigned long long (&n)[2]) const {
        const float4* pl = c.planes + 4u * (size_t)idx;
        const float4 q0 = pl[0], q1 = pl[1], q2 = pl[2];
        const V3 po = mk3(q0.x, q0.y, q0.z), d0 = mk3(q1.x, q1.y, q1.z), d1 = mk3(q2.x, q2.y, q2.z);
        PlaneIts its;
        if (!plane_intersect(po, d0, d1, q0.w, q1.w, cam, rd, kEps, tfar, &its)) return;
        n[0]++;
        // PhotonPlane::contribute (vol_primitives.rs:337-373), then `* norm_photon`
        const V3 p_its = cam + rd * its.t_cam;
        const V3 p0 = po + d0 * its.t0;
        if (!shadow_visible(sc, recs, stack, p0, p_its)) return;
        n[1]++;
        const float4 q3 = pl[3];
        const Col trans = medium_transmittance(sc.medium, its.t_cam);
        const Col sigma_s = mkc(sc.medium.sigma_s[0], sc.medium.sigma_s[1], sc.medium.sigma_s[2]);
        const Col phase_func = cval(div_rn(1.0f, kPi * 4.0f));            // PhaseFunction::Isotropic()
        const float inv_jacobian = div_rn(1.0f, fabsf(dot(d0, cross(d1, -rd))));
        cs = cs + (((((mkc(q3.x, q3.y, q3.z) * phase_func) * sigma_s) * sigma_s) * trans) * inv_jacobian) * c.beam.norm_photon;
    }
};

// beam_gather over two trees: per sample the beam tree, then the plane tree, into one cs
template <bool LDS_SCENE>
RL_DEV void pplane_gather(const RenderConst& rc, const DeviceScene& sc, const StackConf& stc, float4* smem, const PPlaneConst& pc) {
    const BeamLeaf beams{pc.beam};
    const PPlaneLeaf planes{pc};
    SceneRecs recs;
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x;
    const TravStackT<LDS_SCENE> stack = open_scene<LDS_SCENE>(sc, stc, smem, tid, &recs);
    const unsigned ob = blockIdx.x, c = threadIdx.x;
    unsigned bx, by, bw, bh;
    block_geometry(rc, rc.owned_blocks[ob], &bx, &by, &bw, &bh);
    const bool active = c < bw * bh;
    unsigned long long n_entered = 0, n_beam[1] = {}, n_plane[2] = {};
    if (active) {
        Rng rng = rng_seed(rc.block_seeds[rc.owned_blocks[ob]], rc.seed_variant);
        rng_advance<false>(rng, c * rc.spp * 2u);
        const unsigned ix = c / bh, iy = c - (c / bh) * bh;
        const V3 cam = mk3(sc.camera.position[0], sc.camera.position[1], sc.camera.position[2]);
        Col sum = czero();
        for (unsigned s = 0; s < rc.spp; s++) {
            const float u = (float)(bx + ix) + rng_next_f32(rng);         // Point2::new(ix_c + next(), iy_c + next())
            const float v = (float)(by + iy) + rng_next_f32(rng);
            const V3 rd = camera_direction(sc, u, v);
            Hit hit;
            const float tfar = trace_closest(sc, recs, stack, cam, rd, hit) ? hit.t : kF32Max;     // ray.tfar = max_dist; a miss still gathers
            const V3 inv_d = mk3(div_rn(1.0f, rd.x), div_rn(1.0f, rd.y), div_rn(1.0f, rd.z));
            Col cs = czero();
            unsigned i = 0u;
            while (i < pc.beam.n_nodes) {                                   // bvh_beams.gather(&ray)
                const float4 a = pc.beam.nodes[2u * i], b = pc.beam.nodes[2u * i + 1u];
                float te;
                if (!slab(mk3(a.x, a.y, a.z), mk3(a.w, b.x, b.y), cam, inv_d, kEps, tfar, &te)) { i = __float_as_uint(b.z); continue; }
                n_entered++;
                const unsigned fc = __float_as_uint(b.w), first = fc >> 3, count = fc & 7u;
                for (unsigned k = 0; k < count; k++) beams.element(first + k, cam, rd, tfar, sc, recs, stack, cs, n_beam);
                i++;
            }
            i = 0u;
            while (i < pc.n_nodes) {                                        // bvh_planes.gather(&ray)
                const float4 a = pc.nodes[2u * i], b = pc.nodes[2u * i + 1u];
                float te;
                if (!slab(mk3(a.x, a.y, a.z), mk3(a.w, b.x, b.y), cam, inv_d, kEps, tfar, &te)) { i = __float_as_uint(b.z); continue; }
                n_entered++;
                const unsigned fc = __float_as_uint(b.w), first = fc >> 3, count = fc & 7u;
                for (unsigned k = 0; k < count; k++) planes.element(first + k, cam, rd, tfar, sc, recs, stack, cs, n_plane);
                i++;
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
        gather_split24(n_plane[0], &vals[4], &vals[5]);
        gather_split24(n_plane[1], &vals[6], &vals[7]);
        block_stats<8>(rc.partials, rows, vals);
    }
}

template <bool LDS_SCENE>
__global__ void __launch_bounds__(256) k_pplane_gather(RenderConst rc, DeviceScene sc, StackConf stc, PPlaneConst pc) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    pplane_gather<LDS_SCENE>(rc, sc, stc, smem, pc);
}

}  // namespace rl
