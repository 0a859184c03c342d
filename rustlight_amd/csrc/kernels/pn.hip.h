// pn.hip.h — IntegratorPointNormal (src/integrators/explicit/point_normal.rs): single scattering from the lights along the camera ray, the scattering distance
// sampled by transmittance, equi-angularly, equi-angularly clamped to the light's hemisphere, or by the point-normal pdf.  The seven plain strategies (no
// Taylor, warp, "best", MIS, splitting or ATS flavour).  Instantiated by pn_lds.hip (scene staged in LDS) and pn_stream.hip (BVH streamed from L2 / HBM).
//
// compute_pixel (:2585-2633, use_mis = false, splitting = None): 2 draws for the pixel jitter (none with -z: the pixel centre), camera.generate, accel.trace for
// max_dist = Some(its.dist) | None; then compute_single_tr (:2209-2284), compute_single_tr_phase (:2287-2334) or compute_single_strategy (:2336-2453).
//
// Draws per camera sample, in the order they are taken (plus the 2 of the jitter):
//   tr_ex              1 distance, 4 emitter (next, next, next2d)                                  = 5
//   tr_phase           1 distance, 2 phase                                                         = 3
//   eq_ex              4 emitter, 1 distance                                                       = 5
//   eq_phase           4 emitter, 1 distance, 2 phase                                              = 7
//   eq_clamped_ex      4 emitter, then 1 distance only when new_clamping gave Some                 = 4 | 5
//   pn_ex              4 emitter, then 1 distance only when PointNormalSampling::new gave Some     = 4 | 5
//   eq_clamped_phase   4 emitter, then 1 distance + 2 phase only when new_clamping gave Some       = 4 | 7
// Every `return Color::zero()` behind the distance draw comes after all draws of its sample, so only the three strategies whose sampler can be None
// (:2364-2367) take a data-dependent count — decided by the camera ray's closest hit, the emitter sample and a few dot products, and by no other ray.
//
// Where the reference panics, defined here once (the restatement tests/pn_restatement.py says the same):
//   (1) EquiAngularSampling::new asserts theta_a < theta_b (:42); both atans can saturate to one float.  Such a sample takes its usual draws and adds zero.
//   (2) TransmittanceSampling panics when the sampled distance `exited` on an unbounded ray (:1093-1096).  The sample adds zero, with its usual draws.
// Everything else is literal: Color / f32 gives zero on a zero or non-finite divisor, f32::max ignores NaN, signum(+0) = 1 and signum(-0) = -1, crate::clamp
// lets NaN through, theta_b = FRAC_PI_2 - 0.00001 on a miss, the point light's zero normal makes every clamped or point-normal sampler None (d_dot_n = 0 <= 0
// and p_dot_n = 0 >= 0), lights are one-sided (n . (-d) <= 0 adds zero).
//
// Numerics: atan(x) = atan2f_det(x, 1), tan(x) = the IEEE quotient sinf_det(x) / cosf_det(x) (it departs from libm's tan by this construction), powi(2) = x * x.
//
// Drivers, templates over a sample body: PnPlain<STRATEGY> here (k_pn_pixel<LDS_SCENE, PnPlain<STRATEGY>>), PnMis<FAMILY> in pnmis.hip.h, PnTaylor<STRATEGY>
// in pntaylor.hip.h; a body is handed the launch's PnConst, which only PnTaylor reads.  k_pn_pixel: one
// lane per pixel, its samples in series (the pixel sum keeps the reference's order), pixels in compute_mc's order (iy outer, ix inner, mod.rs:420-435); the
// lane's sampler is (a) forked per sample from the pixel's seed (k_seed_pixels), (b) the block's stream entered c * spp * D draws down by rng_advance when the
// count D is constant, (c) the state k_pn_chain recorded for the pixel when it is not; or, as the cross-check of (b) and (c), one lane per block walks the
// block's stream in the reference's order (the form k_pixel_mc has).  k_pn_chain: one lane per block walks (pixel, sample), takes the jitter, the camera
// ray's closest hit and the body's emitter draws (four, or the light tree's three), decides Some | None with pn_make_sampler — the statements the body decides it with — and skips the draws the
// body takes behind them (plain: 1 or 3 | 0); it records the sampler at the start of every pixel (32 bytes per pixel).
#pragma once
#include "light.hip.h"      // light_mesh_position
#include "rngjump.h"        // rng_advance

namespace rl {

static constexpr int kPnWaves = 4;      // 128 VGPRs

RL_DEV bool pn_is_tr(int s) { return s == RL_PN_TR_EX || s == RL_PN_TR_PHASE; }
RL_DEV bool pn_is_phase(int s) { return s == RL_PN_TR_PHASE || s == RL_PN_EQ_PHASE || s == RL_PN_EQ_CLAMPED_PHASE; }
RL_DEV bool pn_is_clamped(int s) { return s == RL_PN_EQ_CLAMPED_EX || s == RL_PN_EQ_CLAMPED_PHASE; }
RL_DEV bool pn_may_fail(int s) { return pn_is_clamped(s) || s == RL_PN_PN_EX; }

RL_DEV float pn_atan(float x) { return dm::atan2f_det(x, 1.0f); }
RL_DEV float pn_tan(float x) { return div_rn(dm::sinf_det(x), dm::cosf_det(x)); }

// fix_random_sample_emitter's non-ATS arm (:1201-1216) / compute_single_tr's (:2244-2254): EmitterSampler::random_sample_emitter_position (emitter.rs:1752-1762),
// then flux * emitter.correct_flux() — 1 / PI for a mesh (emitter.rs:601-603), 1 / (4 PI) for a point light (:243-245)
struct PnEmitter { V3 p, n; Col flux; bool surface; };
RL_DEV PnEmitter pn_sample_emitter(const DeviceScene& sc, float r_sel, float r_pos, V2 uv) {
    const unsigned id = cdf_sample(sc.emitters_cdf, sc.n_emitters + 1, r_sel);
    const float pdf_sel = sc.emitters_cdf[id + 1] - sc.emitters_cdf[id];
    const EmitterRecord em = sc.emitters[id];
    PnEmitter e;
    float correct;
    if (em.kind == EMITTER_MESH) {
        light_mesh_position(sc, sc.meshes[em.mesh], r_pos, uv, &e.p, &e.n, &e.flux);
        e.surface = true;
        correct = div_rn(1.0f, kPi);
    } else {                                                                // PointEmitter::sample_position (emitter.rs:217-229); the host refuses the other kinds
        e.p = mk3(em.v[0], em.v[1], em.v[2]); e.n = mk3(0.0f, 0.0f, 0.0f);
        e.flux = mkc(em.c[0], em.c[1], em.c[2]) * 4.0f * kPi;
        e.surface = false;
        correct = div_rn(1.0f, 4.0f * kPi);
    }
    e.flux = div_unguarded(e.flux, pdf_sel);                                // w / pdf_sel
    e.flux = e.flux * correct;
    return e;
}
// The emitter pick, a policy of the sample bodies: the power pick here, the light tree's PnAtsPick in pnats.hip.h.  kDraws: the draws one pick takes (next,
// next, next2d | next, next2d); on_ray: fix_random_sample_emitter (:1201-1230), at_point: compute_single_tr's pick at the scattering point (:2237-2249)
struct PnPowerPick {
    static constexpr unsigned kDraws = 4;
    static RL_DEV PnPowerPick make(const PnConst&) { return {}; }
    RL_DEV PnEmitter on_ray(const DeviceScene& sc, V3, V3, bool, float, float r_sel, float r_pos, V2 uv) const { return pn_sample_emitter(sc, r_sel, r_pos, uv); }
    RL_DEV PnEmitter at_point(const DeviceScene& sc, V3, float r_sel, float r_pos, V2 uv) const { return pn_sample_emitter(sc, r_sel, r_pos, uv); }
};
// the draws of one pick, in the order they are taken; a pick of three draws has no r_pos
template <unsigned DRAWS>
RL_DEV void pn_emitter_draws(Rng& rng, float* r_sel, float* r_pos, V2* uv) {
    *r_sel = rng_next_f32(rng);
    *r_pos = DRAWS == 4 ? rng_next_f32(rng) : 0.0f;
    *uv = smp_next2d(rng);
}

// EquiAngularSampling (:14-24) and, for pn_ex, PointNormalSampling's a and b (:651-658)
struct PnDist { float delta, d_l, theta_a, theta_b, a, b; };

// create_distance_sampling's three plain arms (:1393, :1547; the transmittance arm :1550 keeps no state): false = None, or the first defined panic
template <int STRATEGY>
RL_DEV bool pn_make_sampler(bool has_max, float max_dist, V3 o, V3 d, V3 pos, V3 n, PnDist* ds) {
    // EquiAngularSampling::new / new_clamping (:27-79)
    const float delta = dot(d, pos - o);
    const float d_l = length(pos - (o + d * delta));
    float theta_a = pn_atan(div_rn(-delta, d_l));
    float theta_b = has_max ? pn_atan(div_rn(max_dist - delta, d_l)) : kPi2 - 0.00001f;
    ds->delta = delta; ds->d_l = d_l; ds->a = 0.0f; ds->b = 0.0f;
    if (!pn_may_fail(STRATEGY)) {
        ds->theta_a = theta_a; ds->theta_b = theta_b;
        return theta_a < theta_b;                                           // assert!(theta_a < theta_b) (:42): defined panic (1)
    }
    // the clamping of the angles (:82-119)
    const float d_dot_n = dot(d, n);
    const float p_dot_n = dot(pos - o, n);
    if (d_dot_n <= 0.0f && p_dot_n >= 0.0f) return false;
    if (!(fabsf(d_dot_n) < 0.00001f || (p_dot_n == 0.0f && d_dot_n > 0.0f))) {
        const float t_hit = div_rn(p_dot_n, d_dot_n);
        if (!(t_hit < 0.0f || t_hit > (has_max ? max_dist : kF32Max))) {
            const float alpha_clamp = pn_atan(div_rn(t_hit - delta, d_l));
            if (p_dot_n > 0.0f) theta_a = alpha_clamp; else theta_b = alpha_clamp;
        }
    }
    ds->theta_a = theta_a; ds->theta_b = theta_b;
    if (theta_a >= theta_b) return false;
    if (STRATEGY != RL_PN_PN_EX) return true;
    // PointNormalSampling::new (:661-703)
    if (theta_b <= theta_a) return false;
    const V3 dv = ((o + d * delta) - pos) / d_l;
    float a = dot(n, dv);
    float b = dot(n, d);
    const float norm = a * (dm::sinf_det(theta_b) - dm::sinf_det(theta_a)) - b * (dm::cosf_det(theta_b) - dm::cosf_det(theta_a));
    ds->a = div_rn(a, norm); ds->b = div_rn(b, norm);
    return !(norm <= 0.0f);
}

// EquiAngularSampling::sample (:146-166)
RL_DEV void pn_sample_equiangular(const PnDist& ds, bool has_max, float max_dist, float sample, float* t_out, float* pdf_out) {
    const float t = ds.d_l * pn_tan((1.0f - sample) * ds.theta_a + sample * ds.theta_b);
    float t_eq = t + ds.delta;
    float pdf = (ds.theta_b - ds.theta_a) * (ds.d_l * ds.d_l + t * t);
    if (pdf != 0.0f) pdf = div_rn(ds.d_l, pdf);
    if (t_eq < 0.0f) t_eq = 0.0f;
    if (has_max && t_eq > max_dist) t_eq = max_dist;
    *t_out = t_eq; *pdf_out = pdf;
}
// PointNormalSampling::sample (:708-739)
RL_DEV void pn_sample_point_normal(const PnDist& ds, float sample, float* t_out, float* pdf_out) {
    const float a = ds.a, b = ds.b;
    const float sa = dm::sinf_det(ds.theta_a), ca = dm::cosf_det(ds.theta_a);
    const float smp = sample + a * sa - b * ca;
    const float v = sqrt_rn(rmax(a * a + b * b - smp * smp, 0.0f));
    const float q = a * smp;
    const float r = div_rn(b * v, signum_f(a));
    const float s = -b * smp;
    const float t = v * fabsf(a);
    const float sol1 = dm::atan2f_det(q + r, s + t);
    float theta = (sol1 >= ds.theta_a && sol1 <= ds.theta_b) ? sol1 : dm::atan2f_det(q - r, s - t);
    theta = theta < ds.theta_a ? ds.theta_a : (theta > ds.theta_b ? ds.theta_b : theta);       // crate::clamp (lib.rs:59-67): a NaN passes
    const float sin_t = dm::sinf_det(theta), cos_t = dm::cosf_det(theta);
    const float td = ds.d_l * div_rn(sin_t, cos_t);
    const float pdf_angular = a * cos_t + b * sin_t;
    const float jacobian = div_rn(ds.d_l, ds.d_l * ds.d_l + td * td);
    *t_out = td + ds.delta; *pdf_out = fabsf(pdf_angular * jacobian);
}
// TransmittanceSampling::sample (:1087-1116); false: defined panic (2)
RL_DEV bool pn_sample_transmittance(const MediumRecord& m, bool has_max, float max_dist, float sample, float* t_out, float* pdf_out) {
    const Col sigma_t = mkc(m.sigma_t[0], m.sigma_t[1], m.sigma_t[2]);
    const float u3 = sample * 3.0f;
    const int component = u3 != u3 ? 0 : (u3 <= 0.0f ? 0 : (u3 >= 255.0f ? 255 : (int)u3));       // `as u8`
    const float u = sample * 3.0f - (float)component;
    const float sigma_t_c = cget(sigma_t, component);
    if (!has_max) {                                                          // HomogenousVolume::sample with tfar = f32::MAX (volume.rs:95-135)
        const float t = div_rn(-m_logf(1.0f - u), sigma_t_c);
        const float t_min = rmin(t, kF32Max);
        const Col tau = t_min * sigma_t;
        *t_out = t_min; *pdf_out = cavg(sigma_t * cexp(-tau));
        return !(t >= kF32Max);
    }
    const float norm = 1.0f - m_expf(-sigma_t_c * max_dist);
    const float t = div_rn(-m_logf(1.0f - u * norm), sigma_t_c);
    const Col norm_c = cval(1.0f) - cexp((-sigma_t) * max_dist);
    *t_out = t; *pdf_out = cavg((sigma_t / norm_c) * cexp((-sigma_t) * t));
    return true;
}

// pn_sample<STRATEGY> — IntegratorPointNormal::compute_pixel for one camera sample of pixel (px, py) on `rng`: the single body every driver calls.
// `aa` (use_aa) is a run-time flag, uniform over the launch: with it as a template argument a kernel holds the body twice, and the explicit strategies then
// spill 10 to 13 VGPRs at 128.  park(rng) is called once, behind the sample's last draw: every draw comes before the sample's second ray, so a driver that
// parks the sampler in memory there carries no sampler through that traversal.
template <int STRATEGY, class Pick, class Stack, class Park>
RL_DEV Col pn_sample(const DeviceScene& sc, const SceneRecs& recs, const Stack& stack, bool aa, unsigned px, unsigned py, Rng& rng, Park&& park,
                     unsigned& n_rays, unsigned& n_vertices, const Pick& pick) {
    float u = (float)px + 0.5f, v = (float)py + 0.5f;
    if (aa) { u = (float)px + rng_next_f32(rng); v = (float)py + rng_next_f32(rng); }
    const V3 o = mk3(sc.camera.position[0], sc.camera.position[1], sc.camera.position[2]);
    const V3 d = camera_direction(sc, u, v);
    Hit hit;
    const bool has_max = trace_closest(sc, recs, stack, o, d, hit);
    const float max_dist = hit.t;
    const MediumRecord& m = sc.medium;
    const Col sigma_s = mkc(m.sigma_s[0], m.sigma_s[1], m.sigma_s[2]);

    float t_cam = 0.0f, t_pdf = 0.0f;
    bool ok = true;
    PnEmitter em;
    V2 s2;
    if (pn_is_tr(STRATEGY)) {
        ok = pn_sample_transmittance(m, has_max, max_dist, rng_next_f32(rng), &t_cam, &t_pdf);
        if (STRATEGY == RL_PN_TR_EX) {
            float r_sel, r_pos; V2 uv;
            pn_emitter_draws<Pick::kDraws>(rng, &r_sel, &r_pos, &uv);
            em = pick.at_point(sc, o + d * t_cam, r_sel, r_pos, uv);
        }
    } else {
        float r_sel, r_pos; V2 uv;
        pn_emitter_draws<Pick::kDraws>(rng, &r_sel, &r_pos, &uv);
        em = pick.on_ray(sc, o, d, has_max, max_dist, r_sel, r_pos, uv);
        PnDist ds;
        ok = pn_make_sampler<STRATEGY>(has_max, max_dist, o, d, em.p, em.n, &ds);
        if (pn_may_fail(STRATEGY) && !ok) { park(rng); return czero(); }    // t_strategy.is_none() (:2364-2367): before the distance draw
        if (ok) n_vertices++;
        const float xi = rng_next_f32(rng);
        if (STRATEGY == RL_PN_PN_EX) pn_sample_point_normal(ds, xi, &t_cam, &t_pdf);
        else pn_sample_equiangular(ds, has_max, max_dist, xi, &t_cam, &t_pdf);
    }
    if (pn_is_phase(STRATEGY)) s2 = smp_next2d(rng);
    park(rng);
    if (!ok) return czero();                                                // the two defined panics: zero, behind the sample's draws
    const V3 p = o + d * t_cam;
    const Col cam_trans = medium_transmittance(m, t_cam) / t_pdf;
    if (pn_is_phase(STRATEGY)) {
        V3 nd; Col weight; float spdf;
        phase_sample(m, -d, s2, &nd, &weight, &spdf);
        Hit h2;
        n_rays++;
        if (!trace_closest(sc, recs, stack, p, nd, h2)) return czero();
        const SurfacePoint nx = fill_intersection(sc, h2.prim, h2.u, h2.v, p, nd, h2.t);
        const MeshRecord nm = sc.meshes[nx.mesh];
        if (!(nm.flags & MESH_IS_LIGHT)) return czero();
        if (dot(nx.n_g, -nd) < 0.0f) return czero();
        const Col contrib = mesh_emit(sc, nm, nx.has_uv, nx.uv) * sigma_s * weight;
        return contrib * cam_trans * medium_transmittance(m, length(nx.p - p));
    }
    V3 d_light = em.p - p;
    const float t_light = length(d_light);
    if (t_light == 0.0f || !finite_f(t_light)) return czero();
    d_light = d_light / t_light;
    const float cos_l = dot(em.n, -d_light);
    const float geom = em.surface ? div_rn(cos_l, t_light * t_light) : div_rn(1.0f, t_light * t_light);
    const Col flux = em.flux * geom;
    if (em.surface && cos_l <= 0.0f) return czero();
    // (the sample's value before its visibility ray: the ray only decides between it and zero, and nothing but the value is kept across the traversal)
    const Col contrib = flux * sigma_s * phase_eval(m, -d, d_light);
    const Col value = contrib * cam_trans * medium_transmittance(m, t_light);
    n_rays++;
    return shadow_visible(sc, recs, stack, p, em.p) ? value : czero();
}

// a sampler parked in memory, [slot][4] u64.  The loads are volatile: a parked state is to be read again, not carried in registers from the store before it
RL_DEV void pn_store_state(unsigned long long* states, unsigned slot, const Rng& r) {
    ulonglong2* q = reinterpret_cast<ulonglong2*>(states + 4 * (size_t)slot);
    q[0] = make_ulonglong2(r.s0, r.s1); q[1] = make_ulonglong2(r.s2, r.s3);
}
RL_DEV Rng pn_load_state(const unsigned long long* states, unsigned slot) {
    const volatile unsigned long long* q = states + 4 * (size_t)slot;
    Rng r; r.s0 = q[0]; r.s1 = q[1]; r.s2 = q[2]; r.s3 = q[3];
    return r;
}

// PnPlain<STRATEGY> — what the drivers below need to know of a sample body, and nothing else (pnmis.hip.h's PnMis<FAMILY> is the other one): the waves per
// SIMD k_pn_pixel is compiled for, the counters a lane carries, the body itself, the statistics rows, and for k_pn_chain the draws a sample takes behind
// its emitter draws.  PnPlainBody is the body over an emitter pick; PnPlain<STRATEGY>, the name the kernels carry, is the one over the power pick.
template <int STRATEGY, class Pick, int WAVES = kPnWaves>
struct PnPlainBody {
    static constexpr int kWaves = WAVES;
    static constexpr unsigned kEmitterDraws = Pick::kDraws;
    struct Counts { unsigned rays = 0, vertices = 0; };
    template <class Stack, class Park>
    static RL_DEV Col sample(const DeviceScene& sc, const SceneRecs& recs, const Stack& stack, bool aa, unsigned px, unsigned py, Rng& rng, Park&& park, Counts& n, const PnConst& pc) {
        return pn_sample<STRATEGY>(sc, recs, stack, aa, px, py, rng, park, n.rays, n.vertices, Pick::make(pc));
    }
    // three rows; the host derives the five counters from them (pn_render.hip.h): a sample's draws follow from its strategy and from whether it had a
    // sampler, n.rays are the phase rays of a phase strategy and the visibility rays of an explicit one, a transmittance sample always has its sampler
    static RL_DEV void stats(const RenderConst& rc, unsigned samples, const Counts& n) {
        const int which[3] = {STAT_SAMPLES, STAT_VERTICES, pn_is_phase(STRATEGY) ? STAT_EXT_RAYS : STAT_SHADOW_RAYS};
        const unsigned vals[3] = {samples, n.vertices, n.rays};
        block_stats<3>(rc.partials, which, vals);
    }
    // Some | None by pn_make_sampler, the statements pn_sample decides it with: 1 or 3 draws behind a sampler, none without
    static RL_DEV unsigned chain_skip(const DeviceScene& sc, bool has_max, float max_dist, V3 o, V3 d, float r_sel, float r_pos, V2 uv, const PnConst& pc) {
        const PnEmitter em = Pick::make(pc).on_ray(sc, o, d, has_max, max_dist, r_sel, r_pos, uv);
        PnDist ds;
        if (!pn_make_sampler<STRATEGY>(has_max, max_dist, o, d, em.p, em.n, &ds)) return 0u;
        return pn_is_phase(STRATEGY) ? 3u : 1u;
    }
};
template <int STRATEGY>
struct PnPlain : PnPlainBody<STRATEGY, PnPowerPick> {};

// k_pn_pixel<LDS_SCENE, Body> — work item = pixel (pc.mode PN_MODE_PER_SAMPLE | _ADVANCE | _GIVEN), or block (PN_MODE_BLOCK: the single-pass walk).
// What a lane keeps between two samples lives in memory, so that the second traversal of a sample runs with its value and little else in registers: the
// sampler in pc.pixel_states[item] (per-sample streams: the pixel's forked sampler; else the block's stream where the pixel stands in it), the pixel's sum in
// the image itself, added to in sample order and scaled behind the last sample.  The kernel itself is the template over the body: a __global__ wrapper per
// body around a shared device function costs a VGPR or two, and tr_phase its fifth wave.
template <bool LDS_SCENE, class Body>
__global__ void __launch_bounds__(256, Body::kWaves) k_pn_pixel(RenderConst rc, DeviceScene sc, StackConf stc, PnConst pc) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneRecs recs;
    const unsigned item = blockIdx.x * blockDim.x + threadIdx.x;
    const TravStackT<LDS_SCENE> stack = open_scene<LDS_SCENE>(sc, stc, smem, item, &recs);
    unsigned n_pix = 0;
    typename Body::Counts counts;
    if (item < rc.n_items) {
        unsigned bx = 0, by = 0, bw = 1;
        n_pix = 1;
        if (pc.mode == PN_MODE_BLOCK) {
            unsigned bh;
            const unsigned b = rc.owned_blocks[item];
            block_geometry(rc, b, &bx, &by, &bw, &bh);
            n_pix = bw * bh;
            pn_store_state(pc.pixel_states, item, rng_seed(rc.block_seeds[b], rc.seed_variant));
        } else {
            const unsigned pix = rc.item_pixel[item];
            bx = pix % rc.W; by = pix / rc.W;
            if (pc.mode == PN_MODE_PER_SAMPLE) pn_store_state(pc.pixel_states, item, rng_seed(rc.item_seed[item], rc.seed_variant));
            else if (pc.mode == PN_MODE_ADVANCE) {
                // the pixel's place c in its block's loop (iy outer, ix inner), c * spp * D draws down the block's stream (the host holds 256 * spp * D to 32 bits)
                const unsigned ox = bx & ~15u, oy = by & ~15u;
                const unsigned c = (by - oy) * min(16u, rc.W - ox) + (bx - ox);
                Rng rng = rng_seed(rc.block_seeds[(ox >> 4) * rc.nby + (oy >> 4)], rc.seed_variant);
                rng_advance<false>(rng, c * rc.spp * pc.draws);
                pn_store_state(pc.pixel_states, item, rng);
            }
        }
        for (unsigned c = 0; c < n_pix; c++) {
            const unsigned px = bx + c % bw, py = by + c / bw;
            volatile float* out = rc.out + 3 * ((size_t)py * rc.W + px);
            out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f;
            for (unsigned s = 0; s < rc.spp; s++) {
                Rng rng = pn_load_state(pc.pixel_states, item);
                if (pc.mode == PN_MODE_PER_SAMPLE) {
                    const unsigned long long seed = rng_next_u64(rng);
                    pn_store_state(pc.pixel_states, item, rng);
                    rng = rng_seed(seed, rc.seed_variant);
                }
                const auto park = [&](const Rng& r) { if (pc.mode != PN_MODE_PER_SAMPLE) pn_store_state(pc.pixel_states, item, r); };
                const Col l = Body::sample(sc, recs, stack, pc.use_aa != 0, px, py, rng, park, counts, pc);
                const float r = out[0] + l.r, g = out[1] + l.g, b = out[2] + l.b;      // im_block.accumulate, in sample order
                out[0] = r; out[1] = g; out[2] = b;
            }
            const float r = out[0] * rc.inv_spp, g = out[1] * rc.inv_spp, b = out[2] * rc.inv_spp;      // im_block.scale(1 / spp)
            out[0] = r; out[1] = g; out[2] = b;
        }
    }
    Body::stats(rc, n_pix * rc.spp, counts);
}

// k_pn_chain<LDS_SCENE, Body> — the bodies whose count depends on the data: one lane per owned block, the chains dealt to every 2^item_shift-th lane as
// k_mc_chain deals them, records where every pixel starts in its block's stream.  Its rays are not counted.
template <bool LDS_SCENE, class Body>
__global__ void __launch_bounds__(256, kPnWaves) k_pn_chain(RenderConst rc, DeviceScene sc, StackConf stc, PnConst pc) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneRecs recs;
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x;
    const TravStackT<LDS_SCENE> stack = open_scene<LDS_SCENE>(sc, stc, smem, tid, &recs);
    const unsigned item = (tid & ((1u << rc.item_shift) - 1u)) == 0u ? (tid >> rc.item_shift) : 0xffffffffu;
    if (item >= rc.n_items) return;
    unsigned bx, by, bw, bh;
    const unsigned b = rc.owned_blocks[item];
    block_geometry(rc, b, &bx, &by, &bw, &bh);
    Rng rng = rng_seed(rc.block_seeds[b], rc.seed_variant);
    const unsigned base = rc.block_item_base[item];
    const V3 o = mk3(sc.camera.position[0], sc.camera.position[1], sc.camera.position[2]);
    for (unsigned c = 0; c < bw * bh; c++) {
        const unsigned px = bx + c % bw, py = by + c / bw;
        pn_store_state(pc.pixel_states, base + c, rng);
        for (unsigned s = 0; s < rc.spp; s++) {
            float u = (float)px + 0.5f, v = (float)py + 0.5f;
            if (pc.use_aa) { u = (float)px + rng_next_f32(rng); v = (float)py + rng_next_f32(rng); }
            const V3 d = camera_direction(sc, u, v);
            Hit hit;
            const bool has_max = trace_closest(sc, recs, stack, o, d, hit);
            float r_sel, r_pos; V2 uv;
            pn_emitter_draws<Body::kEmitterDraws>(rng, &r_sel, &r_pos, &uv);
            const unsigned skip = Body::chain_skip(sc, has_max, hit.t, o, d, r_sel, r_pos, uv, pc);
            for (unsigned k = 0; k < skip; k++) rng_next_u64(rng);
        }
    }
}

template <class F>
static void with_pn_strategy(int strategy, F&& f) {
    switch (strategy) {
        case RL_PN_TR_EX: f(std::integral_constant<int, RL_PN_TR_EX>{}); break;
        case RL_PN_TR_PHASE: f(std::integral_constant<int, RL_PN_TR_PHASE>{}); break;
        case RL_PN_EQ_EX: f(std::integral_constant<int, RL_PN_EQ_EX>{}); break;
        case RL_PN_EQ_PHASE: f(std::integral_constant<int, RL_PN_EQ_PHASE>{}); break;
        case RL_PN_EQ_CLAMPED_EX: f(std::integral_constant<int, RL_PN_EQ_CLAMPED_EX>{}); break;
        case RL_PN_EQ_CLAMPED_PHASE: f(std::integral_constant<int, RL_PN_EQ_CLAMPED_PHASE>{}); break;
        default: f(std::integral_constant<int, RL_PN_PN_EX>{}); break;
    }
}
// chain = true: k_pn_chain (the three data-dependent strategies only; any other strategy launches nothing), false: k_pn_pixel
template <bool LDS_SCENE>
static void launch_pn_impl(bool chain, int strategy, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PnConst& pc) {
    if (!chain) {
        with_pn_strategy(strategy, [&](auto s) { hipLaunchKernelGGL((k_pn_pixel<LDS_SCENE, PnPlain<decltype(s)::value>>), grid, block, lds_bytes, st, rc, ds, stc, pc); });
        return;
    }
    if (strategy == RL_PN_EQ_CLAMPED_EX) hipLaunchKernelGGL((k_pn_chain<LDS_SCENE, PnPlain<RL_PN_EQ_CLAMPED_EX>>), grid, block, lds_bytes, st, rc, ds, stc, pc);
    else if (strategy == RL_PN_EQ_CLAMPED_PHASE) hipLaunchKernelGGL((k_pn_chain<LDS_SCENE, PnPlain<RL_PN_EQ_CLAMPED_PHASE>>), grid, block, lds_bytes, st, rc, ds, stc, pc);
    else if (strategy == RL_PN_PN_EX) hipLaunchKernelGGL((k_pn_chain<LDS_SCENE, PnPlain<RL_PN_PN_EX>>), grid, block, lds_bytes, st, rc, ds, stc, pc);
}

}  // namespace rl
