// uplane.hip.h — IntegratorSinglePlaneUncorrelated (src/integrators/explicit/uncorrelated_plane_single.rs): plane-single's estimate with no plane set — every
// camera sample makes its own nb_primitive planes from the block's stream and tests each against its own ray.  No light pass, no tree, no plane in memory: a
// plane lives in registers between plane_sample and plane_contribution (plane.hip.h).  Instantiated by uplane_lds.hip (scene staged in LDS) and uplane_stream.hip
// (BVH streamed from L2 / HBM).
//
// Per camera sample, in the block's loop order ix, iy, sample (:95-97): 2 draws for the pixel jitter (:99-102), the camera ray with tfar = its closest hit's
// distance or f32::MAX (:103-110); then per plane j < nb_primitive 1 draw for id_emitter (:115; clamped to the last light, plane-single's stated deviation), 1
// more under Average / DiscreteMIS for the plane type — < 1/3 UV, < 2/3 VT, else UT (:142-167): ONE plane of a random type —, and plane_sample's 6 (:44-79), its
// direction drawn again while z == 0.  The plane is then SinglePlane's leaf (:179-292): intersection with tnear = 1e-4, the point on the light, one visibility
// ray, c += w * rho * transmittance * sigma_s * flux * n_lights * (1 / nb_primitive).  Two behaviours of the reference are kept as they are:
//   (1) there is no tree, so a plane with a non-finite corner is not refused: it goes through plane_intersect, whose comparisons let a NaN pass where the
//       reference lets it pass;
//   (2) Average and DiscreteMIS pick one of three plane types with probability 1/3 and still weight it by 1/3 (or by a balance weight that sums to 1 over the
//       types), and divide by nb_primitive: they give a third of the radiance the other strategies give.
//
// The stream.  Workgroup = one owned block, lane c = ix * bh + iy of it, as in beam_gather (gather.hip.h).  Without a redraw a sample takes D = 2 + nb_primitive
// * P draws (P = 7, or 8 with the type draw), so lane c starts c * spp * D draws down the block's stream and walks its samples and planes serially, drawing its
// own directions again in place as the reference does; it counts the extra draws e_c it took, 2 per redraw.  A redraw moves the start of every later lane, which
// the block resolves in rounds: with `first` lanes final and `shift` extra draws before them, the lanes >= first run from c * spp * D + shift; one LDS minimum
// finds the first lane q >= first with e_q > 0; without one every lane >= first commits and the block is done; with one the lanes first .. q commit (nothing
// before q drew again, so they and q itself stood where the reference stands), shift += e_q, first = q + 1, and only the lanes > q run again.  Every round commits
// a lane or ends, so the rounds are bounded by the lanes; every thread of the workgroup, lanes past bw * bh included, reaches every barrier (first, shift and q
// are uniform).  A lane writes its pixel when it commits and never runs again, so the counters it holds at the end are the committed run's.
#pragma once
#include "plane.hip.h"

namespace rl {

static constexpr unsigned kUPlaneNoLane = 256u;      // the LDS minimum when no lane drew again: one past the last lane

template <bool LDS_SCENE, int MODE>
__global__ void __launch_bounds__(256) k_uplane(RenderConst rc, DeviceScene sc, StackConf stc, UPlaneConst uc) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    __shared__ unsigned s_first, s_extra;
    SceneRecs recs;
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x;
    const TravStackT<LDS_SCENE> stack = open_scene<LDS_SCENE>(sc, stc, smem, tid, &recs);
    const unsigned ob = blockIdx.x, c = threadIdx.x;
    unsigned bx, by, bw, bh;
    block_geometry(rc, rc.owned_blocks[ob], &bx, &by, &bw, &bh);
    const bool active = c < bw * bh;
    const unsigned ix = c / bh, iy = c - (c / bh) * bh;
    const V3 cam = mk3(sc.camera.position[0], sc.camera.position[1], sc.camera.position[2]);
    const Col sigma_t = mkc(sc.medium.sigma_t[0], sc.medium.sigma_t[1], sc.medium.sigma_t[2]);
    const Col sigma_s = mkc(sc.medium.sigma_s[0], sc.medium.sigma_s[1], sc.medium.sigma_s[2]);
    const bool pick = MODE == PLANE_MODE_DISCRETE_MIS || (MODE == PLANE_MODE_PLAIN && uc.pick_type != 0);
    unsigned n_samples = 0, n_redraws = 0;
    unsigned long long n_isect = 0, n_visible = 0;
    unsigned shift = 0u, q;
    for (unsigned first = 0u; first < kUPlaneNoLane; first = q + 1u) {
        if (threadIdx.x == 0u) s_first = kUPlaneNoLane;
        __syncthreads();
        const bool run = active && c >= first;
        Col sum = czero();
        if (run) {
            n_samples = 0; n_redraws = 0; n_isect = 0; n_visible = 0;
            Rng rng = rng_seed(rc.block_seeds[rc.owned_blocks[ob]], rc.seed_variant);
#pragma unroll 1
            for (int k = 0; k < 2; k++) rng_advance<false>(rng, k == 0 ? c * rc.spp * uc.draws : shift);     // two jumps: base and shift each stay within 32 bits
            for (unsigned s = 0; s < rc.spp; s++) {
                n_samples++;
                const float u = (float)(bx + ix) + rng_next_f32(rng);         // Point2::new(ix_c + next(), iy_c + next())
                const float v = (float)(by + iy) + rng_next_f32(rng);
                const V3 rd = camera_direction(sc, u, v);
                Hit hit;
                const float tfar = trace_closest(sc, recs, stack, cam, rd, hit) ? hit.t : kF32Max;     // ray.tfar = max_dist
                Col cs = czero();
                for (unsigned j = 0; j < uc.nb_primitive; j++) {
                    unsigned id = (unsigned)(rng_next_f32(rng) * uc.n_lights_f);
                    if (id >= uc.n_lights) id = uc.n_lights - 1u;
                    unsigned type = MODE == PLANE_MODE_CMIS ? (unsigned)RL_PLANE_UALPHAT : uc.type;
                    if (pick) {
                        const float plane_type = rng_next_f32(rng);
                        type = plane_type < 1.0f / 3.0f ? RL_PLANE_UV : plane_type < 2.0f / 3.0f ? RL_PLANE_VT : RL_PLANE_UT;
                    }
                    const PlaneLight& light = uc.lights[id];
                    Plane p; V2 sample;
                    while (!plane_sample(rng, type, light, sigma_t, sigma_s, &p, &sample)) n_redraws++;
                    PlaneIts its;
                    if (!plane_intersect(p.o, p.d0, p.d1, p.l0, p.l1, cam, rd, kEps, tfar, &its)) continue;
                    n_isect++;
                    if (plane_contribution<MODE>(type, p.o, p.d0, p.d1, light, its, cam, rd, sc, recs, stack, uc.w, uc.n_lights_f, uc.inv_nb, [&]() { return p.weight; }, cs))
                        n_visible++;
                }
                sum = sum + cs;                                                 // im_block.accumulate, in sample order
            }
            if (n_redraws) atomicMin(&s_first, c);
        }
        __syncthreads();
        q = s_first;
        if (run && c <= q) {                                                    // commit
            const Col px = scale_unguarded(sum, rc.inv_spp);                    // im_block.scale(1 / spp)
            const size_t pix = (size_t)(by + iy) * rc.W + (bx + ix);
            rc.out[3 * pix] = px.r; rc.out[3 * pix + 1] = px.g; rc.out[3 * pix + 2] = px.b;
        }
        if (c == q) s_extra = 2u * n_redraws;
        __syncthreads();
        if (q == kUPlaneNoLane) break;
        shift += s_extra;
    }
    {
        // extension rays and draws follow from the samples and the redraws on the host
        static constexpr int rows[6] = {STAT_SAMPLES, STAT_UPLANE_REDRAWS, STAT_PLANE_ISECT, STAT_PLANE_ISECT_HI, STAT_PLANE_VISIBLE, STAT_PLANE_VISIBLE_HI};
        unsigned vals[6];
        vals[0] = n_samples; vals[1] = n_redraws;
        gather_split24(n_isect, &vals[2], &vals[3]);
        gather_split24(n_visible, &vals[4], &vals[5]);
        block_stats<6>(rc.partials, rows, vals);
    }
}

template <bool LDS_SCENE>
static void launch_uplane_impl(int mode, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const UPlaneConst& uc) {
    with_plane_mode(mode, [&](auto m) { hipLaunchKernelGGL((k_uplane<LDS_SCENE, decltype(m)::value>), grid, block, lds_bytes, st, rc, ds, stc, uc); });
}

}  // namespace rl
