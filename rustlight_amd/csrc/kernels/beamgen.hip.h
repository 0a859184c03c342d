// beamgen.hip.h — the beam pass of the photon beams (src/integrators/explicit/vol_primitives.rs:437-523, 608-630): the light paths k_vpl_generate and
// k_vpl_shoot walk (vpl.hip.h, vpl_paths.hip.h), stored as beams by convert_beams(false, ..).  Instantiated by beamgen_lds.hip (scene staged in LDS) and
// beamgen_stream.hip (BVH streamed from L2 / HBM).
//
// A beam is an edge that ends in a vertex.  The scene has a medium (the host refuses one without), so every traced edge ends in one (edge.rs:90-126): a path
// stores one beam per extension ray.  Beam: o = the position of the vertex the edge leaves, d = the edge's direction, length = edge.dist (the sampled medium
// distance where the path scattered, the hit distance otherwise), radiance = the flux that reached o (convert_beams pushes, then multiplies by the edge's
// weight * rr_weight on recursion), from_surface = o is the light vertex or a surface vertex.
//
// Record (kBeamWords u32, the layout rl_beam_read documents): [0..2] o, [3] length, [4..6] d, [7] bit 0 = from_surface, [8..10] radiance, [11] the index of
// the path within the generation.
//
// Two kernels over one walk (beam_path): k_beam_generate, one lane on the main sampler's serial stream while fewer than nb_primitive beams are stored (the last
// path's are all kept), and k_beam_shoot, one light path per lane under the stream contract of vpl_paths.hip.h (path k on the k-th clone_box, a count pass and
// a write pass, records in path order and in vertex order within a path).  The draws and their order are k_vpl_generate's.
#pragma once
#include "light.hip.h"      // light_mesh_position
#include "rngjump.h"        // rng_advance

namespace rl {

static constexpr int kBeamWords = RL_BEAM_WORDS;

// one beam record, written with plain vector stores
RL_DEV void beam_store(unsigned* words, unsigned cap, unsigned idx, V3 o, float len, V3 d, bool from_surface, Col radiance, unsigned path) {
    if (idx >= cap) return;
    unsigned w[kBeamWords];
    w[0] = __float_as_uint(o.x); w[1] = __float_as_uint(o.y); w[2] = __float_as_uint(o.z); w[3] = __float_as_uint(len);
    w[4] = __float_as_uint(d.x); w[5] = __float_as_uint(d.y); w[6] = __float_as_uint(d.z); w[7] = from_surface ? 1u : 0u;
    w[8] = __float_as_uint(radiance.r); w[9] = __float_as_uint(radiance.g); w[10] = __float_as_uint(radiance.b); w[11] = path;
    unsigned* dst = words + (size_t)idx * kBeamWords;
#pragma unroll
    for (int k = 0; k < kBeamWords; k++) dst[k] = w[k];
}

// One light path from `rng`: Path::from_light, `generate` with TechniqueVolPrimitives and DirectionalSamplingStrategy { Radiance }, convert_beams(false, ..).
// Beams go to words[n_beams ..] (WRITE) and are counted in n_beams; the other counters are k_vpl_generate's.
template <int MAT, bool LDS_SCENE, bool WRITE>
RL_DEV void beam_path(const RenderConst& rc, const DeviceScene& sc, const SceneRecs& recs, const TravStackT<LDS_SCENE>& stack, Rng& rng, unsigned* words, unsigned cap,
                      unsigned path, unsigned& n_beams, unsigned& n_vertices, unsigned& n_ext, unsigned& n_draws) {
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
    // ---- the light vertex: always expanded (max_depth >= 2 is checked by the host)
    n_vertices++;
    const V2 u2 = smp_next2d(rng);
    n_draws += 2;
    V3 rd; Col w_edge = cone();
    if (em.kind == EMITTER_MESH) {
        const V3 dl = cosine_sample_hemisphere(u2);
        if (dl.z < 0.0f) w_edge = czero();
        rd = to_world(make_frame(ln), dl);
    } else if (em.kind == EMITTER_POINT) rd = sample_uniform_sphere(u2);
    else rd = ln;
    if (is_zero(w_edge)) return;
    Col thr = w_edge;
    float xi = rng_next_f32(rng);
    n_draws++;
    V3 ro = lp;
    float rr = 1.0f;
    unsigned gen = 1u;
    bool from_surface = true;                                      // Vertex::Light
    for (;;) {
        n_ext++;
        Hit hit; hit.t = kF32Max; hit.u = 0.0f; hit.v = 0.0f; hit.prim = -1;
        traverse<false>(recs, sc.root, mk3(sc.root_min[0], sc.root_min[1], sc.root_min[2]), mk3(sc.root_max[0], sc.root_max[1], sc.root_max[2]),
                        ro, rd, kEps, kF32Max, hit, stack);
        const bool is_hit = hit.prim >= 0;
        const MediumSample ms = medium_sample(sc.medium, is_hit ? hit.t : kF32Max, xi);
        w_edge = w_edge * ms.w;
        const bool is_volume = !is_hit || !ms.exited;
        // convert_beams: the beam of this edge carries the flux that reached its first vertex
        if (WRITE) beam_store(words, cap, n_beams, ro, is_volume ? ms.t : hit.t, rd, from_surface, flux, path);
        n_beams++;
        flux = (flux * w_edge) * rr;                               // flux * edge.weight * edge.rr_weight
        V3 vp;
        SurfacePoint sp;
        const Material* mat = nullptr;
        if (is_volume) vp = ro + rd * ms.t;
        else {
            sp = fill_intersection(sc, hit.prim, hit.u, hit.v, ro, rd, hit.t);
            mat = &sc.materials[sc.meshes[sp.mesh].material];
            vp = sp.p;
        }
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
        xi = rng_next_f32(rng);
        n_draws++;
        ro = vp; rd = nd; w_edge = sw; rr = rr_new; gen = gnew; from_surface = !is_volume;
    }
}

// k_beam_generate<MAT, LDS_SCENE> — lane 0 of one workgroup (the others only stage the scene): the loop of vol_primitives.rs:608-630, Beams arm.
// bc: nb_vpl = nb_primitive, cap, max_paths, vpl_words = the beam records, gen_state, gen_out as k_vpl_generate reads and leaves them.
template <int MAT, bool LDS_SCENE>
__global__ void __launch_bounds__(256) k_beam_generate(RenderConst rc, DeviceScene sc, StackConf stc, VplConst bc) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneRecs recs;
    const unsigned tid = threadIdx.x;
    const TravStackT<LDS_SCENE> stack = open_scene<LDS_SCENE>(sc, stc, smem, tid, &recs);
    if (tid != 0u) return;
    Rng rng; rng.s0 = bc.gen_state[0]; rng.s1 = bc.gen_state[1]; rng.s2 = bc.gen_state[2]; rng.s3 = bc.gen_state[3];
    unsigned n_beams = 0, n_paths = 0, n_vertices = 0, n_ext = 0, n_draws = 0;
    while (n_beams < bc.nb_vpl && n_paths < bc.max_paths) {        // still_shoot = beams.len() < self.nb_primitive
        beam_path<MAT, LDS_SCENE, true>(rc, sc, recs, stack, rng, bc.vpl_words, bc.cap, n_paths, n_beams, n_vertices, n_ext, n_draws);
        n_paths++;
    }
    bc.gen_state[0] = rng.s0; bc.gen_state[1] = rng.s1; bc.gen_state[2] = rng.s2; bc.gen_state[3] = rng.s3;
    bc.gen_out[VPL_GEN_VPLS] = n_beams; bc.gen_out[VPL_GEN_PATHS] = n_paths; bc.gen_out[VPL_GEN_VERTICES] = n_vertices;
    bc.gen_out[VPL_GEN_EXT] = n_ext; bc.gen_out[VPL_GEN_DRAWS] = n_draws;
}

// k_beam_shoot<MAT, LDS_SCENE, WRITE> — persistent workgroups as k_vpl_shoot: lane j walks paths first + j, first + j + lanes, ..
template <int MAT, bool LDS_SCENE, bool WRITE>
__global__ void __launch_bounds__(256) k_beam_shoot(RenderConst rc, DeviceScene sc, StackConf stc, VplPathsConst pc) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneRecs recs;
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x;
    const TravStackT<LDS_SCENE> stack = open_scene<LDS_SCENE>(sc, stc, smem, tid, &recs);
    const unsigned lanes = gridDim.x * blockDim.x;
    for (unsigned j = tid; j < pc.count; j += lanes) {
        const unsigned k = pc.first + j;
        // ---- clone_box: the k-th next_u64 of the main sampler seeds the path's stream
        Rng rng; rng.s0 = pc.main[0]; rng.s1 = pc.main[1]; rng.s2 = pc.main[2]; rng.s3 = pc.main[3];
        rng_advance<false>(rng, k);
        rng = rng_seed(rng_next_u64(rng), rc.seed_variant);
        const unsigned base = WRITE ? pc.offsets[k] : 0u;
        unsigned n_beams = base, n_vertices = 0, n_ext = 0, n_draws = 0;
        beam_path<MAT, LDS_SCENE, WRITE>(rc, sc, recs, stack, rng, pc.vpl_words, pc.cap, k, n_beams, n_vertices, n_ext, n_draws);
        if (!WRITE) {                                              // plain vector stores, four unsigned per path
            unsigned* c = pc.counts + 4u * (size_t)j;
            c[VPL_PATH_RECORDS] = n_beams; c[VPL_PATH_VERTICES] = n_vertices; c[VPL_PATH_EXT] = n_ext; c[VPL_PATH_DRAWS] = n_draws;
        }
    }
}

// which: 0 = k_beam_generate, 1 = k_beam_shoot's count pass, 2 = its write pass; vc is read by 0, pc by 1 and 2
template <bool LDS_SCENE>
static void launch_beamgen_impl(int which, int mat, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc,
                                const VplConst& vc, const VplPathsConst& pc) {
    with_bsdf(mat, [&](auto M) {
        constexpr int MAT = decltype(M)::value;
        if (which == 0) hipLaunchKernelGGL((k_beam_generate<MAT, LDS_SCENE>), grid, block, lds_bytes, st, rc, ds, stc, vc);
        else if (which == 1) hipLaunchKernelGGL((k_beam_shoot<MAT, LDS_SCENE, false>), grid, block, lds_bytes, st, rc, ds, stc, pc);
        else hipLaunchKernelGGL((k_beam_shoot<MAT, LDS_SCENE, true>), grid, block, lds_bytes, st, rc, ds, stc, pc);
    });
}

}  // namespace rl
