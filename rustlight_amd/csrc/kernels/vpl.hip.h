// vpl.hip.h — IntegratorVPL (src/integrators/explicit/vpl.rs): virtual point lights shot from the emitters, then gathered at every camera sample.
// Instantiated by vpl_lds.hip (scene staged in LDS) and vpl_stream.hip (BVH streamed from L2 / HBM).  The scene is opened and traced through the helpers
// every secondary kernel uses (stages.hip.h: open_scene, trace_closest, trace_none, shadow_visible) except where a kernel says why it keeps a block
// written out; the light-path walk of k_vpl_generate is k_light_fused's (light.hip.h), restated with Transport::Radiance (bsdf_sample<MAT, true>).
//
// Generation (vpl.rs:182-210): k_vpl_generate, one lane, walks the main sampler's serial stream as the reference does — Path::from_light, `generate`
// with TechniqueVPL and DirectionalSamplingStrategy { transport: Radiance } (the shading-normal correction scales the throughput, which only the
// Russian roulette reads; glass transmission carries eta^2), and convert_vpl on every vertex, while fewer than nb_vpl VPLs are stored (the last path's
// are all kept).  The state of the sampler comes from the host and goes back to it.  At most VplConst::max_paths paths are shot.
//
// Gather (vpl.rs:217-535) in reference-order streams: compute_vpl_contrib always takes D draws (2 jitter draws, + 1 medium draw when the scene has a
// medium), so sample (ix, iy, s) of a block starts at draw ((ix * bh + iy) * spp + s) * D of the block's stream (ix outer, vpl.rs:217).  Per sample
// index s: k_vpl_primary (one lane per pixel, the pixel's stream entered once with rng_advance and kept between passes) traces the camera ray, samples
// the medium and appends the live gather points (ballot / mbcnt compaction); k_vpl_gather (one lane per live point) sums over the VPLs in VPL order and
// adds the sample's radiance to its pixel's sum, which is therefore taken in sample order.  k_vpl_resolve scales the sums by 1 / spp.
//
// VPL record (kVplWords u32, the layout rl_vpl_read documents): [0] kind (VPL_SURFACE, VPL_VOLUME, VPL_EMITTER_POS, VPL_EMITTER_INF), [1] mesh,
// [2] has_uv, [3] 0, [4..6] position (the direction d for VPL_EMITTER_INF), [7..9] radiance, [10..12] wi (surface, local) / d_in (volume) / n (emitter
// position), [13..14] uv, [15..23] the shading frame x, y, z (surface).  Unused words are 0.
#pragma once
#include "light.hip.h"      // light_mesh_position
#include "rngjump.h"        // rng_advance

namespace rl {

static constexpr int kVplWords = RL_VPL_WORDS;
enum { VPL_SURFACE = RL_VPL_KIND_SURFACE, VPL_VOLUME = RL_VPL_KIND_VOLUME, VPL_EMITTER_POS = RL_VPL_KIND_EMITTER_POSITION, VPL_EMITTER_INF = RL_VPL_KIND_EMITTER_INFINITE };
enum { VPL_GP_SURFACE = 1, VPL_GP_VOLUME = 2, VPL_GP_WEIGHTED = 4 };

RL_DEV void vpl_put3(unsigned* w, V3 v) { w[0] = __float_as_uint(v.x); w[1] = __float_as_uint(v.y); w[2] = __float_as_uint(v.z); }
RL_DEV void vpl_putc(unsigned* w, Col c) { w[0] = __float_as_uint(c.r); w[1] = __float_as_uint(c.g); w[2] = __float_as_uint(c.b); }
RL_DEV V3 vpl_get3(const unsigned* w) { return mk3(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2])); }
RL_DEV Col vpl_getc(const unsigned* w) { return mkc(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2])); }

// one VPL record, written with plain vector stores
RL_DEV void vpl_store(const VplConst& vc, unsigned idx, unsigned kind, V3 p, Col radiance, V3 dir, const SurfacePoint* sp) {
    if (idx >= vc.cap) return;
    unsigned w[kVplWords];
#pragma unroll
    for (int k = 0; k < kVplWords; k++) w[k] = 0u;
    w[0] = kind;
    vpl_put3(w + 4, p); vpl_putc(w + 7, radiance); vpl_put3(w + 10, dir);
    if (sp) {
        w[1] = (unsigned)sp->mesh; w[2] = sp->has_uv ? 1u : 0u;
        w[13] = __float_as_uint(sp->uv.x); w[14] = __float_as_uint(sp->uv.y);
        vpl_put3(w + 15, sp->frame.x); vpl_put3(w + 18, sp->frame.y); vpl_put3(w + 21, sp->frame.z);
    }
    unsigned* dst = vc.vpl_words + (size_t)idx * kVplWords;
#pragma unroll
    for (int k = 0; k < kVplWords; k++) dst[k] = w[k];
}

// ------------------------------------------------------------------------------------------
// k_vpl_generate<MAT, LDS_SCENE, MEDIUM> — lane 0 of one workgroup (the others only stage the scene): IntegratorVPL::compute's generation loop
template <int MAT, bool LDS_SCENE, bool MEDIUM>
__global__ void __launch_bounds__(256) k_vpl_generate(RenderConst rc, DeviceScene sc, StackConf stc, VplConst vc) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneRecs recs;
    const unsigned tid = threadIdx.x;
    const TravStackT<LDS_SCENE> stack = open_scene<LDS_SCENE>(sc, stc, smem, tid, &recs);
    if (tid != 0u) return;
    Rng rng; rng.s0 = vc.gen_state[0]; rng.s1 = vc.gen_state[1]; rng.s2 = vc.gen_state[2]; rng.s3 = vc.gen_state[3];
    unsigned n_vpl = 0, n_paths = 0, n_vertices = 0, n_ext = 0, n_draws = 0;
    const bool keep_surface = vc.option_vpl != RL_VPL_VOLUME, keep_volume = vc.option_vpl != RL_VPL_SURFACE;
    while (n_vpl < vc.nb_vpl && n_paths < vc.max_paths) {
        n_paths++;
        // ---- Path::from_light: EmitterSampler::random_sample_emitter_position (emitter.rs:1752-1762), as k_light_fused
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
            if (solid_angle) vpl_store(vc, n_vpl, VPL_EMITTER_POS, lp, flux, ln, nullptr);
            else vpl_store(vc, n_vpl, VPL_EMITTER_INF, rd, flux, mk3(0.0f, 0.0f, 0.0f), nullptr);
            n_vpl++;
        }
        if (is_zero(w_edge)) continue;
        Col thr = w_edge;
        float xi = 0.0f;
        if (MEDIUM) { xi = rng_next_f32(rng); n_draws++; }
        V3 ro = lp;
        float rr = 1.0f;
        unsigned gen = 1u;
        for (;;) {
            n_ext++;
            // (trace_closest of stages.hip.h, written out: called as a function it costs k_vpl_generate<4, true, true> its fourth wave per SIMD)
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
                if (keep_surface && !mat->smooth) { vpl_store(vc, n_vpl, VPL_SURFACE, sp.p, flux, sp.wi, &sp); n_vpl++; }
            } else if (keep_volume) { vpl_store(vc, n_vpl, VPL_VOLUME, vp, flux, -rd, nullptr); n_vpl++; }
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
    vc.gen_state[0] = rng.s0; vc.gen_state[1] = rng.s1; vc.gen_state[2] = rng.s2; vc.gen_state[3] = rng.s3;
    vc.gen_out[VPL_GEN_VPLS] = n_vpl; vc.gen_out[VPL_GEN_PATHS] = n_paths; vc.gen_out[VPL_GEN_VERTICES] = n_vertices;
    vc.gen_out[VPL_GEN_EXT] = n_ext; vc.gen_out[VPL_GEN_DRAWS] = n_draws;
}

// ------------------------------------------------------------------------------------------
// k_vpl_primary<LDS_SCENE, MEDIUM> — workgroup = one owned block, lane c = ix * bh + iy of it (vpl.rs:217-218): sample vc.sample of the pixel.  The first pass
// enters the block stream at draw c * spp * D, later passes go on from the state the previous one left.
template <bool LDS_SCENE, bool MEDIUM>
__global__ void __launch_bounds__(256) k_vpl_primary(RenderConst rc, DeviceScene sc, StackConf stc, VplConst vc) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneRecs recs;
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x;
    const TravStackT<LDS_SCENE> stack = open_scene<LDS_SCENE>(sc, stc, smem, tid, &recs);
    const unsigned ob = blockIdx.x, c = threadIdx.x;
    unsigned bx, by, bw, bh;
    block_geometry(rc, rc.owned_blocks[ob], &bx, &by, &bw, &bh);
    const bool active = c < bw * bh;
    const unsigned item = rc.block_item_base[ob] + c;
    unsigned kind = 0u;
    Hit hit; hit.t = kF32Max; hit.u = 0.0f; hit.v = 0.0f; hit.prim = -1;
    V3 rd = mk3(0.0f, 0.0f, 0.0f);
    Col w = cone();
    float t = 0.0f;
    if (active) {
        Rng rng;
        if (vc.sample == 0u) {
            rng = rng_seed(rc.block_seeds[rc.owned_blocks[ob]], rc.seed_variant);
            rng_advance(rng, c * rc.spp * vc.draws);
            vc.acc[3 * (size_t)item] = 0.0f; vc.acc[3 * (size_t)item + 1] = 0.0f; vc.acc[3 * (size_t)item + 2] = 0.0f;
        } else {
            const unsigned long long* q = vc.pix_state + 4 * (size_t)item;
            rng.s0 = q[0]; rng.s1 = q[1]; rng.s2 = q[2]; rng.s3 = q[3];
        }
        const unsigned ix = c / bh, iy = c - (c / bh) * bh;
        const float u = (float)(bx + ix) + rng_next_f32(rng);         // Point2::new(ix + next(), iy + next())
        const float v = (float)(by + iy) + rng_next_f32(rng);
        rd = camera_direction(sc, u, v);
        const V3 cam = mk3(sc.camera.position[0], sc.camera.position[1], sc.camera.position[2]);
        const bool is_hit = trace_closest(sc, recs, stack, cam, rd, hit);
        t = hit.t;
        if (MEDIUM) {
            const float xi = rng_next_f32(rng);                          // taken on every branch (vpl.rs:470, 492)
            const MediumSample ms = medium_sample(sc.medium, is_hit ? hit.t : kF32Max, xi);
            w = ms.w;
            if (is_hit && !ms.exited) { kind = VPL_GP_VOLUME | VPL_GP_WEIGHTED; t = ms.t; }
            else if (is_hit && vc.option_lt != RL_VPL_VOLUME) kind = VPL_GP_SURFACE | VPL_GP_WEIGHTED;
            // a miss inside the medium: the reference's `l_i *= ..` with l_i = 0 (vpl.rs:483) — +0 here, no gather
        } else if (is_hit && vc.option_lt != RL_VPL_SURFACE) kind = VPL_GP_SURFACE;   // the inverted test of vpl.rs:527
        unsigned long long* q = vc.pix_state + 4 * (size_t)item;
        q[0] = rng.s0; q[1] = rng.s1; q[2] = rng.s2; q[3] = rng.s3;
    }
    // the live gather points, compacted: one atomic per wave, lanes in ballot order
    const unsigned long long live = __ballot(kind != 0u);
    const unsigned lane = __builtin_amdgcn_mbcnt_hi((unsigned)(live >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)live, 0u));
    unsigned base = 0u;
    if (live != 0ull) {
        const unsigned first = (unsigned)__builtin_ctzll(live);
        if ((threadIdx.x & 63u) == first) base = atomicAdd(vc.n_live, (unsigned)__popcll(live));
        base = __shfl(base, (int)first, 64);
    }
    if (kind != 0u) {
        unsigned g[kVplGatherWords];
        g[0] = item; g[1] = kind; g[2] = (unsigned)hit.prim; g[3] = __float_as_uint(hit.u); g[4] = __float_as_uint(hit.v); g[5] = __float_as_uint(t);
        vpl_put3(g + 6, rd); vpl_putc(g + 9, w);
        unsigned* dst = vc.gpoints + (size_t)(base + lane) * kVplGatherWords;
#pragma unroll
        for (int k = 0; k < kVplGatherWords; k++) dst[k] = g[k];
    }
    {
        const int which[3] = {STAT_SAMPLES, STAT_EXT_RAYS, STAT_DRAWS};
        const unsigned vals[3] = {active ? 1u : 0u, active ? 1u : 0u, active ? vc.draws : 0u};
        block_stats<3>(rc.partials, which, vals);
    }
}

template <bool MEDIUM>
RL_DEV Col vpl_transmittance(const DeviceScene& sc, float dist) { return MEDIUM ? medium_transmittance(sc.medium, dist) : cone(); }

// ------------------------------------------------------------------------------------------
// k_vpl_gather<MAT, LDS_SCENE, MEDIUM> — one lane per live gather point of this sample: gathering_surface / gathering_volume (vpl.rs:268-442) over all
// VPLs in order; the VPL index is wave-uniform, so its record is read through scalar loads.  No connection ray is traced where it could add nothing
// (a smooth gather point).
template <int MAT, bool LDS_SCENE, bool MEDIUM>
__global__ void __launch_bounds__(256) k_vpl_gather(RenderConst rc, DeviceScene sc, StackConf stc, VplConst vc) {
    // (open_scene of stages.hip.h, written out: called as a function it makes k_vpl_gather<0, true, false> spill four more SGPRs)
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneRecs recs;
    float4* after_scene = smem;
    if (LDS_SCENE) {
        stage_scene_lds(sc, smem, smem + lds_nodes_float4s(sc.n_nodes));
        recs.nodes = smem; recs.tris = smem + lds_nodes_float4s(sc.n_nodes);
        after_scene = smem + lds_scene_float4s(sc.n_nodes, sc.n_prims);
    } else {
        recs.nodes = streamed_nodes<TravStackT<false>>(sc);
        recs.tris = reinterpret_cast<const float4*>(sc.tris);
    }
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x;
    const TravStackT<LDS_SCENE> stack = make_stack<LDS_SCENE>(stc, reinterpret_cast<unsigned*>(after_scene), tid);
    const bool active = tid < *vc.n_live;
    unsigned n_shadow = 0, n_surface = 0, n_volume = 0;
    if (active) {
        const unsigned* g = vc.gpoints + (size_t)tid * kVplGatherWords;
        const unsigned item = g[0], kind = g[1];
        const V3 rd = vpl_get3(g + 6);
        const Col w = vpl_getc(g + 9);
        const V3 cam = mk3(sc.camera.position[0], sc.camera.position[1], sc.camera.position[2]);
        const float norm = vc.norm_vpl;
        Col l = czero();
        if (kind & VPL_GP_SURFACE) {                                   // gathering_surface (vpl.rs:268-380)
            n_surface++;
            const SurfacePoint sp = fill_intersection(sc, (int)g[2], __uint_as_float(g[3]), __uint_as_float(g[4]), cam, rd, __uint_as_float(g[5]));
            const MeshRecord& mr = sc.meshes[sp.mesh];
            const Material& mat = sc.materials[mr.material];
            if (sp.wi.z > 0.0f) l = l + mesh_emit(sc, mr, sp.has_uv, sp.uv);
            if (!mat.smooth) {
                for (unsigned i = 0; i < vc.n_vpl; i++) {
                    const unsigned* r = vc.vpls + (size_t)__builtin_amdgcn_readfirstlane(i) * kVplWords;
                    const unsigned vk = r[0];
                    const V3 vpos = vpl_get3(r + 4);
                    const Col rad = vpl_getc(r + 7);
                    if (vk == VPL_EMITTER_INF) {
                        n_shadow++;
                        if (trace_none(sc, recs, stack, sp.p, -vpos)) {
                            const Col f = bsdf_eval<MAT>(sc, mat, sp.has_uv, sp.uv, sp.wi, to_local(sp.frame, -vpos), false);
                            l = l + (norm * rad) * f;
                        }
                        continue;
                    }
                    if (vk != VPL_VOLUME) {
                        n_shadow++;
                        if (!shadow_visible(sc, recs, stack, vpos, sp.p)) continue;
                    }
                    V3 d = vpos - sp.p;
                    const float dist = length(d);
                    d = d / dist;
                    const Col trans = vpl_transmittance<MEDIUM>(sc, length(vpos - sp.p));
                    const Col f = bsdf_eval<MAT>(sc, mat, sp.has_uv, sp.uv, sp.wi, to_local(sp.frame, d), false);
                    const V3 v3 = vpl_get3(r + 10);
                    if (vk == VPL_EMITTER_POS) {
                        const Col er = (rad * rmax(dot(v3, -d), 0.0f)) * kInvPi;
                        l = l + (((trans * norm) * er) * f) / (dist * dist);
                    } else if (vk == VPL_VOLUME) {
                        const Col er = phase_eval(sc.medium, v3, d);
                        l = l + ((((trans * norm) * er) * f) * rad) / (dist * dist);
                    } else {
                        Frame fr; fr.x = vpl_get3(r + 15); fr.y = vpl_get3(r + 18); fr.z = vpl_get3(r + 21);
                        V2 vuv; vuv.x = __uint_as_float(r[13]); vuv.y = __uint_as_float(r[14]);
                        const Material& vmat = sc.materials[sc.meshes[r[1]].material];
                        const Col er = bsdf_eval<MAT>(sc, vmat, r[2] != 0u, vuv, v3, to_local(fr, -d), false);
                        l = l + ((((trans * norm) * er) * f) * rad) / (dist * dist);
                    }
                }
            }
        } else {                                                       // gathering_volume (vpl.rs:382-442)
            n_volume++;
            const V3 pos = cam + rd * __uint_as_float(g[5]);
            const V3 d_cam = -rd;
            for (unsigned i = 0; i < vc.n_vpl; i++) {
                const unsigned* r = vc.vpls + (size_t)__builtin_amdgcn_readfirstlane(i) * kVplWords;
                const unsigned vk = r[0];
                const V3 vpos = vpl_get3(r + 4);
                const Col rad = vpl_getc(r + 7);
                if (vk != VPL_VOLUME) {                                // (no VPL_EMITTER_INF: a directional light with a medium is refused)
                    n_shadow++;
                    if (!shadow_visible(sc, recs, stack, vpos, pos)) continue;
                }
                V3 d = vpos - pos;
                const float dist = length(d);
                d = d / dist;
                const Col trans = vpl_transmittance<MEDIUM>(sc, length(vpos - pos));
                const Col pv = phase_eval(sc.medium, d_cam, d);
                const V3 v3 = vpl_get3(r + 10);
                if (vk == VPL_EMITTER_POS) {
                    const Col er = (rad * rmax(dot(v3, -d), 0.0f)) * kInvPi;
                    l = l + (((trans * norm) * er) * pv) / (dist * dist);
                } else if (vk == VPL_VOLUME) {
                    const Col er = phase_eval(sc.medium, v3, d);
                    l = l + ((((trans * norm) * er) * pv) * rad) / (dist * dist);
                } else {
                    Frame fr; fr.x = vpl_get3(r + 15); fr.y = vpl_get3(r + 18); fr.z = vpl_get3(r + 21);
                    V2 vuv; vuv.x = __uint_as_float(r[13]); vuv.y = __uint_as_float(r[14]);
                    const Material& vmat = sc.materials[sc.meshes[r[1]].material];
                    const Col er = bsdf_eval<MAT>(sc, vmat, r[2] != 0u, vuv, v3, to_local(fr, -d), false);
                    l = l + ((((trans * norm) * er) * pv) * rad) / (dist * dist);
                }
            }
        }
        const Col L = (kind & VPL_GP_WEIGHTED) ? czero() + l * w : czero() + l;     // l_i += gathering(..) [* mrec.w]
        float* a = vc.acc + 3 * (size_t)item;
        a[0] = a[0] + L.r; a[1] = a[1] + L.g; a[2] = a[2] + L.b;        // im_block.accumulate, in sample order (one pass per sample)
    }
    {
        const int which[3] = {STAT_SHADOW_RAYS, STAT_VPL_SURFACE, STAT_VPL_VOLUME};
        const unsigned vals[3] = {n_shadow, n_surface, n_volume};
        block_stats<3>(rc.partials, which, vals);
    }
}

// which: 0 = k_vpl_generate, 1 = k_vpl_gather, 2 = k_vpl_primary (mat not read)
template <bool LDS_SCENE>
static void launch_vpl_impl(int which, int mat, bool medium, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const VplConst& vc) {
    with_flag(medium, [&](auto MED) {
        constexpr bool MEDIUM = decltype(MED)::value;
        if (which == 2) { hipLaunchKernelGGL((k_vpl_primary<LDS_SCENE, MEDIUM>), grid, block, lds_bytes, st, rc, ds, stc, vc); return; }
        with_bsdf(mat, [&](auto M) {
            if (which == 0) hipLaunchKernelGGL((k_vpl_generate<decltype(M)::value, LDS_SCENE, MEDIUM>), grid, block, lds_bytes, st, rc, ds, stc, vc);
            else hipLaunchKernelGGL((k_vpl_gather<decltype(M)::value, LDS_SCENE, MEDIUM>), grid, block, lds_bytes, st, rc, ds, stc, vc);
        });
    });
}

}  // namespace rl
