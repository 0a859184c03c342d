// pplanegen.hip.h — the plane pass of the photon planes (src/integrators/explicit/vol_primitives.rs:376-523, 608-630, `Planes` arm): the light paths k_beam_generate
// and k_beam_shoot walk (beamgen.hip.h), stored as convert_beams(true, ..) and convert_planes(..) store them.  Instantiated by pplanegen_lds.hip (scene staged in
// LDS) and pplanegen_stream.hip (BVH streamed from L2 / HBM).
//
// A light path is a chain, so what an edge becomes is known one step after it is traced.  An edge that leaves the light vertex or a surface vertex is a beam.  An
// edge e that leaves a volume vertex V1 is a beam when its end vertex V2 is on a surface or was not expanded (depth limit, Russian roulette, zero
// throughput), and a plane when V2 is a volume vertex that was expanded with an edge e2: o = V1, d0 = e.d, d1 = e2.d,
// length0 = continued_t(e) = e.dist (e scattered), length1 = continued_t(e2), the distance e2's medium sample drew before it was cut at the hit distance
// (medium_ct.hip.h), radiance = the flux that reached V1.  An edge from a volume vertex into the medium is therefore held back (`pend`) until the next edge is
// traced (a plane) or the walk ends (a beam).  Beams are in edge order and planes are in edge order, each in its own array.
//
// Records: beams as beamgen.hip.h stores them (kBeamWords u32, rl_beam_read's layout); planes kPlaneWords u32 in rl_plane_read's geometry layout: [0..2] o,
// [3..5] d0, [6..8] d1, [9] length0, [10] length1, [11..13] radiance, [14] the index of the path within the generation, [15] the index of e within the path,
// [16..17] 0.  All stores are plain vector stores.
//
// Two kernels over one walk (pplane_path): k_pplane_generate, one lane on the main sampler's serial stream while fewer than nb_primitive planes are stored (the
// last path's records are all kept), and k_pplane_shoot, one light path per lane under the stream contract of vpl_paths.hip.h (a count pass and a write pass;
// both counts go into the prefix sums; records in path order).  The draws and their order are k_vpl_generate's.
#pragma once
#include "light.hip.h"      // light_mesh_position
#include "rngjump.h"        // rng_advance
#include "beamgen.hip.h"    // beam_store
#include "medium_ct.hip.h"  // medium_sample_ct

namespace rl {

static constexpr int kPlaneWords = RL_PLANE_WORDS;

RL_DEV void pplane_store(unsigned* words, unsigned cap, unsigned idx, V3 o, V3 d0, V3 d1, float l0, float l1, Col radiance, unsigned path, unsigned edge) {
    if (idx >= cap) return;
    unsigned w[kPlaneWords];
    w[0] = __float_as_uint(o.x); w[1] = __float_as_uint(o.y); w[2] = __float_as_uint(o.z);
    w[3] = __float_as_uint(d0.x); w[4] = __float_as_uint(d0.y); w[5] = __float_as_uint(d0.z);
    w[6] = __float_as_uint(d1.x); w[7] = __float_as_uint(d1.y); w[8] = __float_as_uint(d1.z);
    w[9] = __float_as_uint(l0); w[10] = __float_as_uint(l1);
    w[11] = __float_as_uint(radiance.r); w[12] = __float_as_uint(radiance.g); w[13] = __float_as_uint(radiance.b);
    w[14] = path; w[15] = edge; w[16] = 0u; w[17] = 0u;
    unsigned* dst = words + (size_t)idx * kPlaneWords;
#pragma unroll
    for (int k = 0; k < kPlaneWords; k++) dst[k] = w[k];
}

// where one path's records go: planes to planes[n_planes ..], beams to beams[n_beams ..], each behind its own capacity
struct PPlaneOut { unsigned* planes; unsigned plane_cap; unsigned* beams; unsigned beam_cap; };

// One light path from `rng`: beam_path's walk (beamgen.hip.h), stored by convert_beams(true, ..) and convert_planes(..)
template <int MAT, bool LDS_SCENE, bool WRITE>
RL_DEV void pplane_path(const RenderConst& rc, const DeviceScene& sc, const SceneRecs& recs, const TravStackT<LDS_SCENE>& stack, Rng& rng, const PPlaneOut& out,
                        unsigned path, unsigned& n_planes, unsigned& n_beams, unsigned& n_vertices, unsigned& n_ext, unsigned& n_draws) {
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
    // ---- the light vertex: always expanded (max_depth >= 4 is checked by the host)
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
    unsigned gen = 1u, edge = 0u;
    bool from_surface = true;                                      // Vertex::Light
    // the edge held back: it left a volume vertex and ended in one
    bool pend = false;
    V3 pend_o = lp, pend_d = rd; float pend_len = 0.0f; Col pend_flux = czero(); unsigned pend_edge = 0u;
    for (;;) {
        n_ext++;
        Hit hit; hit.t = kF32Max; hit.u = 0.0f; hit.v = 0.0f; hit.prim = -1;
        traverse<false>(recs, sc.root, mk3(sc.root_min[0], sc.root_min[1], sc.root_min[2]), mk3(sc.root_max[0], sc.root_max[1], sc.root_max[2]),
                        ro, rd, kEps, kF32Max, hit, stack);
        const bool is_hit = hit.prim >= 0;
        const MediumSampleCt ms = medium_sample_ct(sc.medium, is_hit ? hit.t : kF32Max, xi);
        w_edge = w_edge * ms.w;
        const bool is_volume = !is_hit || !ms.exited;
        // convert_planes: the held edge's end vertex was expanded with this edge
        if (pend) {
            if (WRITE) pplane_store(out.planes, out.plane_cap, n_planes, pend_o, pend_d, rd, pend_len, ms.continued_t, pend_flux, path, pend_edge);
            n_planes++;
            pend = false;
        }
        // convert_beams(true, ..): from the light or a surface always; from the medium onto a surface; from the medium into the medium once the walk says which
        if (from_surface || !is_volume) {
            if (WRITE) beam_store(out.beams, out.beam_cap, n_beams, ro, is_volume ? ms.t : hit.t, rd, from_surface, flux, path);
            n_beams++;
        } else { pend = true; pend_o = ro; pend_d = rd; pend_len = ms.t; pend_flux = flux; pend_edge = edge; }
        edge++;
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
    // the held edge's end vertex was not expanded: a beam after all, the path's last
    if (pend) {
        if (WRITE) beam_store(out.beams, out.beam_cap, n_beams, pend_o, pend_len, pend_d, false, pend_flux, path);
        n_beams++;
    }
}

// k_pplane_generate<MAT, LDS_SCENE> — lane 0 of one workgroup (the others only stage the scene): the loop of vol_primitives.rs:608-630, Planes arm.
// bc as k_beam_generate reads and leaves it, over the planes (nb_vpl = nb_primitive, cap, vpl_words = the plane records); xc: the beams.  The loop also ends once
// more than xc.beam_max beams are stored (the host refuses the set); gen_out has PPLANE_GEN_WORDS words, gen_out[PPLANE_GEN_BEAMS] = beams stored.
template <int MAT, bool LDS_SCENE>
__global__ void __launch_bounds__(256) k_pplane_generate(RenderConst rc, DeviceScene sc, StackConf stc, VplConst bc, PPlaneGenConst xc) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneRecs recs;
    const unsigned tid = threadIdx.x;
    const TravStackT<LDS_SCENE> stack = open_scene<LDS_SCENE>(sc, stc, smem, tid, &recs);
    if (tid != 0u) return;
    Rng rng; rng.s0 = bc.gen_state[0]; rng.s1 = bc.gen_state[1]; rng.s2 = bc.gen_state[2]; rng.s3 = bc.gen_state[3];
    const PPlaneOut out{bc.vpl_words, bc.cap, xc.beam_words, xc.beam_cap};
    unsigned n_planes = 0, n_beams = 0, n_paths = 0, n_vertices = 0, n_ext = 0, n_draws = 0;
    while (n_planes < bc.nb_vpl && n_paths < bc.max_paths && n_beams <= xc.beam_max) {      // still_shoot = planes.len() < self.nb_primitive
        pplane_path<MAT, LDS_SCENE, true>(rc, sc, recs, stack, rng, out, n_paths, n_planes, n_beams, n_vertices, n_ext, n_draws);
        n_paths++;
    }
    bc.gen_state[0] = rng.s0; bc.gen_state[1] = rng.s1; bc.gen_state[2] = rng.s2; bc.gen_state[3] = rng.s3;
    bc.gen_out[VPL_GEN_VPLS] = n_planes; bc.gen_out[VPL_GEN_PATHS] = n_paths; bc.gen_out[VPL_GEN_VERTICES] = n_vertices;
    bc.gen_out[VPL_GEN_EXT] = n_ext; bc.gen_out[VPL_GEN_DRAWS] = n_draws; bc.gen_out[PPLANE_GEN_BEAMS] = n_beams;
}

// k_pplane_shoot<MAT, LDS_SCENE, WRITE> — persistent workgroups as k_beam_shoot: lane j walks paths first + j, first + j + lanes, ..; the count pass writes
// PPLANE_PATH_WORDS words per path, k_beam_shoot's four and the path's beams at PPLANE_PATH_BEAMS
template <int MAT, bool LDS_SCENE, bool WRITE>
__global__ void __launch_bounds__(256) k_pplane_shoot(RenderConst rc, DeviceScene sc, StackConf stc, VplPathsConst pc, PPlaneGenConst xc) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneRecs recs;
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x;
    const TravStackT<LDS_SCENE> stack = open_scene<LDS_SCENE>(sc, stc, smem, tid, &recs);
    const unsigned lanes = gridDim.x * blockDim.x;
    const PPlaneOut out{pc.vpl_words, pc.cap, xc.beam_words, xc.beam_cap};
    for (unsigned j = tid; j < pc.count; j += lanes) {
        const unsigned k = pc.first + j;
        // ---- clone_box: the k-th next_u64 of the main sampler seeds the path's stream
        Rng rng; rng.s0 = pc.main[0]; rng.s1 = pc.main[1]; rng.s2 = pc.main[2]; rng.s3 = pc.main[3];
        rng_advance<false>(rng, k);
        rng = rng_seed(rng_next_u64(rng), rc.seed_variant);
        const unsigned plane_base = WRITE ? pc.offsets[k] : 0u, beam_base = WRITE ? xc.beam_offsets[k] : 0u;
        unsigned n_planes = plane_base, n_beams = beam_base, n_vertices = 0, n_ext = 0, n_draws = 0;
        pplane_path<MAT, LDS_SCENE, WRITE>(rc, sc, recs, stack, rng, out, k, n_planes, n_beams, n_vertices, n_ext, n_draws);
        if (!WRITE) {                                              // plain vector stores, PPLANE_PATH_WORDS unsigned per path
            unsigned* c = pc.counts + (size_t)PPLANE_PATH_WORDS * j;
            c[VPL_PATH_RECORDS] = n_planes; c[VPL_PATH_VERTICES] = n_vertices; c[VPL_PATH_EXT] = n_ext; c[VPL_PATH_DRAWS] = n_draws; c[PPLANE_PATH_BEAMS] = n_beams;
        }
    }
}

// which: 0 = k_pplane_generate, 1 = k_pplane_shoot's count pass, 2 = its write pass; vc is read by 0, pc by 1 and 2
template <bool LDS_SCENE>
static void launch_pplanegen_impl(int which, int mat, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc,
                                  const VplConst& vc, const VplPathsConst& pc, const PPlaneGenConst& xc) {
    with_bsdf(mat, [&](auto M) {
        constexpr int MAT = decltype(M)::value;
        if (which == 0) hipLaunchKernelGGL((k_pplane_generate<MAT, LDS_SCENE>), grid, block, lds_bytes, st, rc, ds, stc, vc, xc);
        else if (which == 1) hipLaunchKernelGGL((k_pplane_shoot<MAT, LDS_SCENE, false>), grid, block, lds_bytes, st, rc, ds, stc, pc, xc);
        else hipLaunchKernelGGL((k_pplane_shoot<MAT, LDS_SCENE, true>), grid, block, lds_bytes, st, rc, ds, stc, pc, xc);
    });
}

}  // namespace rl
