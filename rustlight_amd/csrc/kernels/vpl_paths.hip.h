// vpl_paths.hip.h — light-path generation on per-path sampler streams (rl_vpl_generate_paths): what k_vpl_generate (vpl.hip.h) walks serially on one
// lane, walked one light path per lane.  Instantiated by vpl_paths_lds.hip (scene staged in LDS) and vpl_paths_stream.hip (BVH streamed from L2 / HBM).
//
// The stream contract.  Light path k = 0, 1, 2, .. draws from the sampler the k-th clone_box() call on the main sampler returns (samplers/independent.rs:
// 18-22): seed_k = the k-th next_u64() of the main sampler counted from its incoming state, the path's stream = rng_seed(seed_k, seed_variant).  Inside its
// stream a path draws exactly what a path of the serial pass draws (light.hip.h lists the order).  A lane reaches seed_k with rng_advance<false>(main, k) and
// one next_u64: nothing it computes depends on which lane, workgroup, batch or launch walks the path.
//
// The host (wavefront.hip: rl_vpl_generate_paths) runs rounds.  A count pass (WRITE = false) walks a batch of consecutive path indices and stores per path
// four unsigned: the records that pass the option filter, the expanded vertices, the extension rays and the draws.  The host takes the prefix sum of the
// record counts and finds K, the smallest path count that stores at least nb_vpl records — the reference's `while stored < nb` on this path sequence.  The
// write pass (WRITE = true) walks paths 0 .. K-1 again and stores each path's records from its own offset, so the records stand in path order and in vertex
// order within a path whatever the arrival order.  Paths beyond K leave nothing behind.
//
// The walk is k_vpl_generate's, restated (not shared: a call costs k_vpl_generate<4, true, true> a wave per SIMD, vpl.hip.h); record layout and option
// filter are its own (vpl_store).
#pragma once
#include "vpl.hip.h"        // vpl_store, the record kinds

namespace rl {

// k_vpl_shoot<MAT, LDS_SCENE, MEDIUM, WRITE> — persistent workgroups: each opens the scene once, then lane j walks paths first + j, first + j + lanes, ..
template <int MAT, bool LDS_SCENE, bool MEDIUM, bool WRITE>
__global__ void __launch_bounds__(256) k_vpl_shoot(RenderConst rc, DeviceScene sc, StackConf stc, VplPathsConst pc) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneRecs recs;
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x;
    const TravStackT<LDS_SCENE> stack = open_scene<LDS_SCENE>(sc, stc, smem, tid, &recs);
    VplConst vc{};
    vc.cap = pc.cap; vc.vpl_words = pc.vpl_words;
    const bool keep_surface = pc.option_vpl != RL_VPL_VOLUME, keep_volume = pc.option_vpl != RL_VPL_SURFACE;
    const unsigned lanes = gridDim.x * blockDim.x;
    for (unsigned j = tid; j < pc.count; j += lanes) {
        const unsigned k = pc.first + j;
        // ---- clone_box: the k-th next_u64 of the main sampler seeds the path's stream
        Rng rng; rng.s0 = pc.main[0]; rng.s1 = pc.main[1]; rng.s2 = pc.main[2]; rng.s3 = pc.main[3];
        rng_advance<false>(rng, k);
        rng = rng_seed(rng_next_u64(rng), rc.seed_variant);
        unsigned n_vpl = WRITE ? pc.offsets[k] : 0u;
        unsigned n_vertices = 0, n_ext = 0, n_draws = 0;
        // ---- Path::from_light: EmitterSampler::random_sample_emitter_position (emitter.rs:1752-1762), as k_vpl_generate
        const float r_sel = rng_next_f32(rng);
        const float r_pos = rng_next_f32(rng);
        const V2 uv = smp_next2d(rng);
        n_draws += 4;
        const unsigned id = cdf_sample(sc.emitters_cdf, sc.n_emitters + 1, r_sel);
        const float pdf_sel = sc.emitters_cdf[id + 1] - sc.emitters_cdf[id];
        const EmitterRecord em = sc.emitters[id];
        V3 lp, ln; Col flux;
        if (em.kind == EMITTER_MESH) light_mesh_position(sc, sc.meshes[em.mesh], r_pos, uv, &lp, &ln, &flux);
        else if (em.kind == EMITTER_POINT) {
            lp = mk3(em.v[0], em.v[1], em.v[2]); ln = mk3(0.0f, 0.0f, 0.0f);
            flux = mkc(em.c[0], em.c[1], em.c[2]) * 4.0f * kPi;
        } else {
            const V2 dp = concentric_sample_disk(uv);
            const float area = kPi * powi_f(em.radius, 2);
            const V3 dir = mk3(em.v[0], em.v[1], em.v[2]);
            const V3 poff = to_world(make_frame(dir), mk3(dp.x, dp.y, 0.0f) * em.radius);
            lp = (mk3(em.center[0], em.center[1], em.center[2]) - dir * em.radius) + poff;
            ln = dir;
            flux = mkc(em.c[0], em.c[1], em.c[2]) * area;
        }
        flux = div_unguarded(flux, pdf_sel);
        // ---- the light vertex: always expanded (max_depth >= 2 is checked by the host); its edge decides the emitter VPL's kind
        n_vertices++;
        const V2 u2 = smp_next2d(rng);
        n_draws += 2;
        V3 rd; Col w_edge = cone(); bool solid_angle = true;
        if (em.kind == EMITTER_MESH) {
            const V3 dl = cosine_sample_hemisphere(u2);
            if (dl.z < 0.0f) w_edge = czero();
            rd = to_world(make_frame(ln), dl);
        } else if (em.kind == EMITTER_POINT) rd = sample_uniform_sphere(u2);
        else { rd = ln; solid_angle = false; }
        if (keep_surface) {                                            // convert_vpl, Vertex::Light (vpl.rs:128-152)
            if (WRITE) {
                if (solid_angle) vpl_store(vc, n_vpl, VPL_EMITTER_POS, lp, flux, ln, nullptr);
                else vpl_store(vc, n_vpl, VPL_EMITTER_INF, rd, flux, mk3(0.0f, 0.0f, 0.0f), nullptr);
            }
            n_vpl++;
        }
        if (!is_zero(w_edge)) {
            Col thr = w_edge;
            float xi = 0.0f;
            if (MEDIUM) { xi = rng_next_f32(rng); n_draws++; }
            V3 ro = lp;
            float rr = 1.0f;
            unsigned gen = 1u;
            for (;;) {
                n_ext++;
                Hit hit; hit.t = kF32Max; hit.u = 0.0f; hit.v = 0.0f; hit.prim = -1;
                traverse<false>(recs, sc.root, mk3(sc.root_min[0], sc.root_min[1], sc.root_min[2]), mk3(sc.root_max[0], sc.root_max[1], sc.root_max[2]),
                                ro, rd, kEps, kF32Max, hit, stack);
                const bool is_hit = hit.prim >= 0;
                bool is_volume = false;
                V3 vp = mk3(0.0f, 0.0f, 0.0f);
                if (MEDIUM) {
                    const MediumSample ms = medium_sample(sc.medium, is_hit ? hit.t : kF32Max, xi);
                    w_edge = w_edge * ms.w;
                    is_volume = !is_hit || !ms.exited;
                    if (is_volume) vp = ro + rd * ms.t;
                } else if (!is_hit) break;
                flux = (flux * w_edge) * rr;                               // flux * edge.weight * edge.rr_weight
                SurfacePoint sp;
                const Material* mat = nullptr;
                if (!is_volume) {
                    sp = fill_intersection(sc, hit.prim, hit.u, hit.v, ro, rd, hit.t);
                    mat = &sc.materials[sc.meshes[sp.mesh].material];
                    vp = sp.p;
                    if (keep_surface && !mat->smooth) { if (WRITE) vpl_store(vc, n_vpl, VPL_SURFACE, sp.p, flux, sp.wi, &sp); n_vpl++; }
                } else if (keep_volume) { if (WRITE) vpl_store(vc, n_vpl, VPL_VOLUME, vp, flux, -rd, nullptr); n_vpl++; }
                // ---- expand: DirectionalSamplingStrategy::bounce with Transport::Radiance (strategies/directional.rs:44-153)
                const unsigned gnew = gen + 1u;
                if (!((rc.has_max ? gnew < rc.max_depth : true) && gnew < kDepthCap)) break;
                n_vertices++;
                const V2 s2 = smp_next2d(rng);
                n_draws += 2;
                V3 nd; Col sw;
                if (is_volume) { float spdf; phase_sample(sc.medium, -rd, s2, &nd, &sw, &spdf); thr = thr * sw; }
                else {
                    BsdfSample bs;
                    if (!bsdf_sample<MAT, true>(sc, *mat, sp.has_uv, sp.uv, sp.wi, s2, &bs)) break;
                    sw = bs.weight; nd = to_world(sp.frame, bs.d);
                    thr = thr * sw;
                    const V3 wi_world = to_world(sp.frame, sp.wi);
                    const float correction = div_rn(sp.wi.z * dot(nd, sp.n_g), bs.d.z * dot(wi_world, sp.n_g));
                    thr = scale_unguarded(thr, fabsf(correction));        // *throughput *= correction.abs() (directional.rs:61-66)
                }
                if (is_zero(thr)) break;
                float rr_new = 1.0f;
                if (rc.has_rr ? rc.rr_depth <= gnew : true) {
                    const float q = rmin(channel_max(thr), 0.95f);
                    const float x = rng_next_f32(rng);
                    n_draws++;
                    if (q < x) break;
                    rr_new = div_rn(1.0f, q);
                }
                thr = scale_unguarded(thr, rr_new);
                if (MEDIUM) { xi = rng_next_f32(rng); n_draws++; }
                ro = vp; rd = nd; w_edge = sw; rr = rr_new; gen = gnew;
            }
        }
        if (!WRITE) {                                                  // plain vector stores, four unsigned per path
            unsigned* c = pc.counts + 4u * (size_t)j;
            c[VPL_PATH_RECORDS] = n_vpl; c[VPL_PATH_VERTICES] = n_vertices; c[VPL_PATH_EXT] = n_ext; c[VPL_PATH_DRAWS] = n_draws;
        }
    }
}

template <bool LDS_SCENE>
static void launch_vpl_paths_impl(bool write, int mat, bool medium, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const VplPathsConst& pc) {
    with_flag(medium, [&](auto MED) {
        with_flag(write, [&](auto WR) {
            with_bsdf(mat, [&](auto M) {
                hipLaunchKernelGGL((k_vpl_shoot<decltype(M)::value, LDS_SCENE, decltype(MED)::value, decltype(WR)::value>), grid, block, lds_bytes, st, rc, ds, stc, pc);
            });
        });
    });
}

}  // namespace rl
