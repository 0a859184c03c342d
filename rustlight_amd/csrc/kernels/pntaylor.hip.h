// pntaylor.hip.h — IntegratorPointNormal's six Taylor strategies (src/integrators/explicit/point_normal.rs): the scattering angle sampled from a degree-six
// Taylor polynomial of the transmittance or of the Henyey-Greenstein phase function about theta = 0, inverted numerically, up to a clamp angle, and uniformly
// (eq, eq_clamped) or by the point-normal pdf (pn) beyond it.  PnTaylor<STRATEGY> is a sample body of pn.hip.h's drivers k_pn_pixel and k_pn_chain;
// instantiated by pntaylor_lds.hip and pntaylor_stream.hip.  The warp and "best" flavours are not built (roots::find_roots_cubic is not in the reference's tree).
//
// compute_single_strategy's EX arm (:2336-2453) over create_distance_sampling's Taylor arms (:1276-1290, :1404-1418): Poly6::{phase, tr, pdf, cdf, cdf_pn}
// (point_normal_poly.rs:178-393), clamp_angle_tr / clamp_angle_phase (:391-399), TaylorSampling::{new, sample} (:401-518), PointNormalTaylorSampling::{new,
// sample} with warp = None (:757-976), math::newton_raphson_iterate (math.rs:136-225).  Poly6::tr_phase, PolyClamped, Poly4 and HybridSampling are not built.
//
// Draws per camera sample, behind the 2 of the jitter (none with -z): 4 emitter (the light tree's pick, pnats.hip.h: 3), then 1 distance only when the sampler is Some.  TaylorSampling::new and
// PointNormalTaylorSampling::new return None on norm <= 0, norm_poly_pn <= 0 or norm_poly <= 0, so every strategy's count depends on the data and every
// strategy takes the chain pass, which decides Some | None with pntaylor_make, the statements the body decides it with.
//
// eq_phase_taylor_ex and eq_clamped_phase_taylor_ex in an Isotropic medium are plain eq_ex / eq_clamped_ex by the reference's text (:1278): the host sends them
// to rl_render_point_normal's kernels.  pn_phase_taylor_ex with g = 0 meets assert!(g != 0.0) (:1414) at every sample: the host refuses it.
//
// Definitions (tests/pntaylor_restatement.py says the same):
//   powi is powi_f, __powisf2's order of products.  Float literals are rounded to f32.  Poly6's sums are evaluated left to right as written.
//   newton_raphson_iterate's factor is 2^-9: (1 - digits) as i32 wraps in a release build (digits = 10 is a usize).
//   A solver that reports div_zero makes sample() return (0, 0): the sample goes on from t_cam = 0 and the guarded Color / 0 gives zero.
//   NaN goes through every comparison literally; f32::min ignores NaN; dbg! and warn! do nothing.
//   tan, atan and crate::clamp are pn.hip.h's; exp is expf_det; sigma_t.avg() is (r + g + b) / 3 in that order.
//   EquiAngularSampling::new's assert!(theta_a < theta_b) (:42), pn.hip.h's defined panic (1), is None here: no distance draw, zero.
//
// Hoisted, the arithmetic unchanged: Poly6::phase(g) and clamp_angle_phase(g) depend on the frame only and come in PnConst::taylor (pntaylor_render.hip.h
// computes them with these statements on the host); cdf_pn's fourteen derived coefficients and its two terms at min_theta are made once per inversion.
#pragma once
#include "pn.hip.h"

namespace rl {

RL_DEV bool pntaylor_is_phase(int s) { return s == RL_PN_TAYLOR_EQ_PHASE || s == RL_PN_TAYLOR_EQ_CLAMPED_PHASE || s == RL_PN_TAYLOR_PN_PHASE; }
RL_DEV bool pntaylor_is_pn(int s) { return s == RL_PN_TAYLOR_PN_TR || s == RL_PN_TAYLOR_PN_PHASE; }

// poly6 (point_normal_poly.rs:178-185)
RL_DEV float poly6_eval(const float* c, float x) {
    return c[0] + c[1] * x + c[2] * x * x + c[3] * x * x * x + c[4] * x * x * x * x + c[5] * x * x * x * x * x + c[6] * x * x * x * x * x * x;
}
struct Poly6 {
    float t[7];
    RL_DEV float pdf(float x) const { return poly6_eval(t, x); }
    // Poly6::cdf (:345-353)
    RL_DEV float cdf(float x) const {
        return x * (t[0] + div_rn(t[1] * x, 2.0f) + div_rn(t[2] * x * x, 3.0f) + div_rn(t[3] * x * x * x, 4.0f) + div_rn(t[4] * x * x * x * x, 5.0f) +
                    div_rn(t[5] * x * x * x * x * x, 6.0f) + div_rn(t[6] * x * x * x * x * x * x, 7.0f));
    }
};
// Poly6::tr (:285-338) with c0 = 1: x = d_norm * sigma_t
RL_DEV Poly6 poly6_tr(float d_norm, float sigma_t) {
    const float x = d_norm * sigma_t;
    Poly6 p;
    p.t[0] = 1.0f;
    p.t[1] = -x;
    p.t[2] = div_rn(x * (-1.0f + x), 2.0f);
    p.t[3] = div_rn(-(x * (-2.0f + x) * (-1.0f + x)), 6.0f);
    p.t[4] = div_rn(x * (-5.0f + x * (11.0f + x * (-6.0f + x))), 24.0f);
    p.t[5] = div_rn(-(x * (16.0f + x * (-45.0f + x * (35.0f + x * (-10.0f + x))))), 120.0f);
    p.t[6] = div_rn(x * (-61.0f + x * (211.0f + x * (-210.0f + x * (85.0f + x * (-15.0f + x))))), 720.0f);
    return p;
}
// clamp_angle_tr (:391-394)
RL_DEV float pntaylor_clamp_angle_tr(float sigma_t, float d_l) { return dm::expf_det(0.210824f - 0.15974f * d_l * sigma_t); }

// Poly6::cdf_pn (:355-392) with its coefficients and its min_theta terms made once: at(max_theta) is the reference's final expression
struct Poly6CdfPn {
    float c1[7], c2[7], p2c, p4s;
    RL_DEV Poly6CdfPn(const Poly6& p, float a, float b, float min_theta) {
        const float* t = p.t;
        c1[0] = -(b * t[0]) + a * t[1] - 6.0f * a * (t[3] - 20.0f * t[5]) + 2.0f * b * (t[2] - 12.0f * t[4] + 360.0f * t[6]);
        c1[1] = -(b * t[1]) + 2.0f * a * t[2] + 6.0f * b * (t[3] - 20.0f * t[5]) - 24.0f * a * (t[4] - 30.0f * t[6]);
        c1[2] = -(b * t[2]) + 3.0f * a * t[3] - 60.0f * a * t[5] + 12.0f * b * (t[4] - 30.0f * t[6]);
        c1[3] = -(b * t[3]) + 4.0f * a * t[4] + 20.0f * b * t[5] - 120.0f * a * t[6];
        c1[4] = -(b * t[4]) + 5.0f * a * t[5] + 30.0f * b * t[6];
        c1[5] = -(b * t[5]) + 6.0f * a * t[6];
        c1[6] = -(b * t[6]);
        c2[0] = a * t[0] + b * t[1] - 6.0f * b * (t[3] - 20.0f * t[5]) - 2.0f * a * (t[2] - 12.0f * t[4] + 360.0f * t[6]);
        c2[1] = a * t[1] + 2.0f * b * t[2] - 6.0f * a * (t[3] - 20.0f * t[5]) - 24.0f * b * (t[4] - 30.0f * t[6]);
        c2[2] = a * t[2] + 3.0f * b * t[3] - 60.0f * b * t[5] - 12.0f * a * (t[4] - 30.0f * t[6]);
        c2[3] = a * t[3] + 4.0f * b * t[4] - 20.0f * a * t[5] - 120.0f * b * t[6];
        c2[4] = a * t[4] + 5.0f * b * t[5] - 30.0f * a * t[6];
        c2[5] = a * t[5] + 6.0f * b * t[6];
        c2[6] = a * t[6];
        p2c = poly6_eval(c1, min_theta) * dm::cosf_det(min_theta);
        p4s = poly6_eval(c2, min_theta) * dm::sinf_det(min_theta);
    }
    RL_DEV float at(float max_theta) const {
        return poly6_eval(c1, max_theta) * dm::cosf_det(max_theta) - p2c + poly6_eval(c2, max_theta) * dm::sinf_det(max_theta) - p4s;
    }
};

// math::newton_raphson_iterate (math.rs:136-225) with max_iter = 30 and digits = 10; f_both(pos, &f, &f_derv).  Returns div_zero; *pos_io is res.pos
template <class F>
RL_DEV bool pntaylor_newton(float* pos_io, float min, float max, float y, F&& f_both) {
    float pos = *pos_io;
    const float factor = 0.001953125f;                                      // scalbn(1.0, -9)
    float delta = kF32Max, delta1 = kF32Max;
    int count = 30;
    bool div_zero = false;
    for (;;) {
        float fv, f1;
        f_both(pos, &fv, &f1);
        const float f0 = fv - y;
        const float delta2 = delta1;
        delta1 = delta;
        count -= 1;
        if (0.0f == f0) break;
        if (f1 == 0.0f) { div_zero = true; break; }
        delta = div_rn(f0, f1);
        if (fabsf(delta * 2.0f) > fabsf(delta2)) delta = delta > 0.0f ? div_rn(pos - min, 2.0f) : div_rn(pos - max, 2.0f);
        const float old_pos = pos;
        pos -= delta;
        if (pos <= min) {
            delta = 0.5f * (old_pos - min);
            pos = old_pos - delta;
            if (pos == min || pos == max) break;
        } else if (pos >= max) {
            delta = 0.5f * (old_pos - max);
            pos = old_pos - delta;
            if (pos == min || pos == max) break;
        }
        if (delta > 0.0f) max = old_pos; else min = old_pos;
        if (count == 0 || fabsf(pos * factor) >= fabsf(delta)) break;
    }
    *pos_io = pos;
    return div_zero;
}

// TaylorSampling (:401-408) or PointNormalTaylorSampling (:757-768) behind their `new`: eq keeps norm and cdf_a, pn keeps a, b (pn.a, pn.b as new leaves
// them), other_a, other_b and norm (norm_poly)
struct PnTaylorDist {
    float delta, d_l, theta_a, theta_b, clamp_angle, prob_poly, norm, cdf_a, a, b, other_a, other_b;
    Poly6 poly;
};

// create_distance_sampling's Taylor arms (:1276-1290, :1404-1418): false = None
template <int STRATEGY>
RL_DEV bool pntaylor_make(const MediumRecord& m, const PnConst& pc, bool has_max, float max_dist, V3 o, V3 d, V3 pos, V3 n, PnTaylorDist* ts) {
    PnDist ds;
    constexpr int kBase = STRATEGY == RL_PN_TAYLOR_EQ_PHASE || STRATEGY == RL_PN_TAYLOR_EQ_TR ? RL_PN_EQ_EX : RL_PN_EQ_CLAMPED_EX;
    if (!pn_make_sampler<kBase>(has_max, max_dist, o, d, pos, n, &ds)) return false;      // new_clamping gave None | defined panic (1)
    const float theta_a = ds.theta_a, theta_b = ds.theta_b;
    ts->delta = ds.delta; ts->d_l = ds.d_l; ts->theta_a = theta_a; ts->theta_b = theta_b;
    ts->norm = 0.0f; ts->cdf_a = 0.0f; ts->a = 0.0f; ts->b = 0.0f; ts->other_a = 0.0f; ts->other_b = 0.0f;
    float pn_a = 0.0f, pn_b = 0.0f, pn_norm = 0.0f;
    if (pntaylor_is_pn(STRATEGY)) {                                          // PointNormalSampling::new (:673-702)
        if (theta_b <= theta_a) return false;
        const V3 dv = ((o + d * ds.delta) - pos) / ds.d_l;
        const float a = dot(n, dv);
        const float b = dot(n, d);
        pn_norm = a * (dm::sinf_det(theta_b) - dm::sinf_det(theta_a)) - b * (dm::cosf_det(theta_b) - dm::cosf_det(theta_a));
        pn_a = div_rn(a, pn_norm); pn_b = div_rn(b, pn_norm);
        if (pn_norm <= 0.0f) return false;
    }
    float clamp_angle;
    if (pntaylor_is_phase(STRATEGY)) {
        for (int i = 0; i < 7; i++) ts->poly.t[i] = pc.taylor[i];
        clamp_angle = pc.taylor[7];
    } else {
        const float sigma_t = cavg(mkc(m.sigma_t[0], m.sigma_t[1], m.sigma_t[2]));
        ts->poly = poly6_tr(ds.d_l, sigma_t);
        clamp_angle = pntaylor_clamp_angle_tr(sigma_t, ds.d_l);
    }
    const Poly6& poly = ts->poly;
    if (!pntaylor_is_pn(STRATEGY)) {                                         // TaylorSampling::new (:411-454)
        float prob_poly = 0.0f, norm = 0.0f, cdf_a = 0.0f;
        if (theta_a > clamp_angle) {
            clamp_angle = theta_a;
        } else if (theta_b > clamp_angle) {
            cdf_a = poly.cdf(theta_a);
            norm = poly.cdf(clamp_angle) - cdf_a;
            if (norm <= 0.0f) return false;
            const float cdf_other = poly.pdf(clamp_angle) * (theta_b - clamp_angle);
            prob_poly = div_rn(norm, norm + cdf_other);
        } else {
            cdf_a = poly.cdf(theta_a);
            norm = poly.cdf(theta_b) - cdf_a;
            clamp_angle = theta_b;
            if (norm <= 0.0f) return false;
            prob_poly = 1.0f;
        }
        ts->clamp_angle = clamp_angle; ts->prob_poly = prob_poly; ts->norm = norm; ts->cdf_a = cdf_a;
        return true;
    }
    // PointNormalTaylorSampling::new (:782-856)
    float other_a, other_b, prob_poly, norm_poly;
    if (theta_a > clamp_angle) {
        clamp_angle = theta_a;
        other_a = pn_a; other_b = pn_b; prob_poly = 0.0f; norm_poly = 0.0f;
    } else if (theta_b > clamp_angle) {
        const float a = pn_a * pn_norm, b = pn_b * pn_norm;
        const float sc_ = dm::sinf_det(clamp_angle), cc = dm::cosf_det(clamp_angle);
        const float norm_new = a * (dm::sinf_det(theta_b) - sc_) - b * (dm::cosf_det(theta_b) - cc);
        other_a = div_rn(a, norm_new); other_b = div_rn(b, norm_new);
        const float norm_poly_pn = a * (sc_ - dm::sinf_det(theta_a)) - b * (cc - dm::cosf_det(theta_a));
        pn_a = div_rn(a, norm_poly_pn); pn_b = div_rn(b, norm_poly_pn);
        if (norm_poly_pn <= 0.0f) return false;
        norm_poly = Poly6CdfPn(poly, pn_a, pn_b, theta_a).at(clamp_angle);
        const float pdf_clamped = (pn_a * cc + pn_b * sc_) * poly.pdf(clamp_angle);
        const float cdf_other = pdf_clamped * (theta_b - clamp_angle);
        prob_poly = div_rn(norm_poly, norm_poly + cdf_other);
    } else {
        norm_poly = Poly6CdfPn(poly, pn_a, pn_b, theta_a).at(theta_b);
        if (norm_poly <= 0.0f) return false;
        other_a = 0.0f; other_b = 0.0f; prob_poly = 1.0f;
    }
    ts->clamp_angle = clamp_angle; ts->prob_poly = prob_poly; ts->norm = norm_poly; ts->a = pn_a; ts->b = pn_b; ts->other_a = other_a; ts->other_b = other_b;
    return true;
}

// TaylorSampling::sample (:458-513)
RL_DEV void pntaylor_sample_eq(const PnTaylorDist& ts, float sample, float* t_out, float* pdf_out) {
    float theta1, pdf_angular;
    if (sample < ts.prob_poly) {
        const float y = div_rn(sample, ts.prob_poly);
        float pos = (ts.clamp_angle + ts.theta_a) * 0.5f;
        const bool div_zero = pntaylor_newton(&pos, ts.theta_a, ts.clamp_angle, y, [&](float v, float* f, float* f1) {
            *f = div_rn(ts.poly.cdf(v) - ts.cdf_a, ts.norm);
            *f1 = div_rn(ts.poly.pdf(v), ts.norm);
        });
        if (div_zero) { *t_out = 0.0f; *pdf_out = 0.0f; return; }
        theta1 = pos;
        pdf_angular = div_rn(ts.prob_poly * ts.poly.pdf(pos), ts.norm);
    } else {
        const float s = div_rn(sample - ts.prob_poly, 1.0f - ts.prob_poly);
        const float range = ts.theta_b - ts.clamp_angle;
        theta1 = range * s + ts.clamp_angle;
        pdf_angular = div_rn(1.0f, range) * (1.0f - ts.prob_poly);
    }
    const float t = ts.d_l * pn_tan(theta1);
    const float jacobian = div_rn(ts.d_l, powi_f(ts.d_l, 2) + powi_f(t, 2));
    *t_out = t + ts.delta; *pdf_out = pdf_angular * jacobian;
}
// PointNormalTaylorSampling::sample with warp = None (:860-971)
RL_DEV void pntaylor_sample_pn(const PnTaylorDist& ts, float sample, float* t_out, float* pdf_out) {
    float theta1, pdf_angular;
    if (sample < ts.prob_poly) {
        const float clamped_theta_b = rmin(ts.theta_b, ts.clamp_angle);
        const float y = div_rn(sample, ts.prob_poly);
        float pos = (clamped_theta_b + ts.theta_a) * 0.5f;
        const Poly6CdfPn cdf_pn(ts.poly, ts.a, ts.b, ts.theta_a);
        const bool div_zero = pntaylor_newton(&pos, ts.theta_a, clamped_theta_b, y, [&](float v, float* f, float* f1) {
            *f = div_rn(cdf_pn.at(v), ts.norm);
            *f1 = div_rn(ts.poly.pdf(v) * (ts.a * dm::cosf_det(v) + ts.b * dm::sinf_det(v)), ts.norm);
        });
        if (div_zero) { *t_out = 0.0f; *pdf_out = 0.0f; return; }
        const float cos_theta = ts.a * dm::cosf_det(pos) + ts.b * dm::sinf_det(pos);
        theta1 = pos;
        pdf_angular = div_rn(ts.prob_poly * ts.poly.pdf(pos) * cos_theta, ts.norm);
    } else {
        const float s = div_rn(sample - ts.prob_poly, 1.0f - ts.prob_poly);
        const float a = ts.other_a, b = ts.other_b, cta = ts.clamp_angle;
        const float smp = s + a * dm::sinf_det(cta) - b * dm::cosf_det(cta);
        const float v = sqrt_rn(rmax(a * a + b * b - powi_f(smp, 2), 0.0f));
        const float q = a * smp;
        const float r = div_rn(b * v, signum_f(a));
        const float sv = -b * smp;
        const float t = v * fabsf(a);
        const float sol1 = dm::atan2f_det(q + r, sv + t);
        const float sol = (sol1 >= cta && sol1 <= ts.theta_b) ? sol1 : dm::atan2f_det(q - r, sv - t);
        theta1 = sol < ts.theta_a ? ts.theta_a : (sol > ts.theta_b ? ts.theta_b : sol);
        pdf_angular = (1.0f - ts.prob_poly) * (a * dm::cosf_det(sol) + b * dm::sinf_det(sol));
    }
    theta1 = theta1 < ts.theta_a ? ts.theta_a : (theta1 > ts.theta_b ? ts.theta_b : theta1);
    const float t = ts.d_l * pn_tan(theta1);
    const float jacobian = div_rn(ts.d_l, powi_f(ts.d_l, 2) + powi_f(t, 2));
    *t_out = t + ts.delta; *pdf_out = pdf_angular * jacobian;
}

// compute_pixel for one camera sample of pixel (px, py) with a Taylor strategy: pn_sample's explicit arm behind another distance sampler
template <int STRATEGY, class Pick, class Stack, class Park>
RL_DEV Col pntaylor_sample(const DeviceScene& sc, const SceneRecs& recs, const Stack& stack, const PnConst& pc, unsigned px, unsigned py, Rng& rng, Park&& park,
                           unsigned& n_rays, unsigned& n_vertices, const Pick& pick) {
    float u = (float)px + 0.5f, v = (float)py + 0.5f;
    if (pc.use_aa != 0) { u = (float)px + rng_next_f32(rng); v = (float)py + rng_next_f32(rng); }
    const V3 o = mk3(sc.camera.position[0], sc.camera.position[1], sc.camera.position[2]);
    const V3 d = camera_direction(sc, u, v);
    Hit hit;
    const bool has_max = trace_closest(sc, recs, stack, o, d, hit);
    const float max_dist = hit.t;
    const MediumRecord& m = sc.medium;
    const Col sigma_s = mkc(m.sigma_s[0], m.sigma_s[1], m.sigma_s[2]);
    float r_sel, r_pos; V2 uv;
    pn_emitter_draws<Pick::kDraws>(rng, &r_sel, &r_pos, &uv);
    const PnEmitter em = pick.on_ray(sc, o, d, has_max, max_dist, r_sel, r_pos, uv);
    float t_cam, t_pdf;
    {
        PnTaylorDist ts;
        if (!pntaylor_make<STRATEGY>(m, pc, has_max, max_dist, o, d, em.p, em.n, &ts)) { park(rng); return czero(); }      // t_strategy.is_none() (:2364-2367)
        n_vertices++;
        const float xi = rng_next_f32(rng);
        park(rng);
        if (pntaylor_is_pn(STRATEGY)) pntaylor_sample_pn(ts, xi, &t_cam, &t_pdf);
        else pntaylor_sample_eq(ts, xi, &t_cam, &t_pdf);
    }
    const V3 p = o + d * t_cam;
    const Col cam_trans = medium_transmittance(m, t_cam) / t_pdf;
    V3 d_light = em.p - p;
    const float t_light = length(d_light);
    if (t_light == 0.0f || !finite_f(t_light)) return czero();
    d_light = d_light / t_light;
    const float cos_l = dot(em.n, -d_light);
    const float geom = em.surface ? div_rn(cos_l, t_light * t_light) : div_rn(1.0f, t_light * t_light);
    const Col flux = em.flux * geom;
    if (em.surface && cos_l <= 0.0f) return czero();
    const Col contrib = flux * sigma_s * phase_eval(m, -d, d_light);
    const Col value = contrib * cam_trans * medium_transmittance(m, t_light);
    n_rays++;
    return shadow_visible(sc, recs, stack, p, em.p) ? value : czero();
}

// PnTaylor<STRATEGY> — the sample body of the Taylor strategies for pn.hip.h's drivers (what PnPlain<STRATEGY> is for the plain ones): PnTaylorBody over the
// power pick
// waves per SIMD k_pn_pixel is compiled for (profiles/pntaylor_note.md records what the compiler reported at four and at three)
// pn_phase_taylor_ex spills 10 VGPRs (48 bytes of scratch) at four and is compiled for three; the other five fit four (121 to 128 VGPRs)
constexpr int pntaylor_waves(int strategy) { return strategy == RL_PN_TAYLOR_PN_PHASE ? 3 : kPnWaves; }
template <int STRATEGY, class Pick, int WAVES = pntaylor_waves(STRATEGY)>
struct PnTaylorBody {
    static constexpr int kWaves = WAVES;
    static constexpr unsigned kEmitterDraws = Pick::kDraws;
    struct Counts { unsigned rays = 0, vertices = 0; };
    template <class Stack, class Park>
    static RL_DEV Col sample(const DeviceScene& sc, const SceneRecs& recs, const Stack& stack, bool, unsigned px, unsigned py, Rng& rng, Park&& park, Counts& n,
                             const PnConst& pc) {
        return pntaylor_sample<STRATEGY>(sc, recs, stack, pc, px, py, rng, park, n.rays, n.vertices, Pick::make(pc));
    }
    // three rows; the host derives the five counters from them (pntaylor_render.hip.h): a sample takes one draw behind its emitter draws when it had a
    // sampler, n.rays are the visibility rays
    static RL_DEV void stats(const RenderConst& rc, unsigned samples, const Counts& n) {
        const int which[3] = {STAT_SAMPLES, STAT_VERTICES, STAT_SHADOW_RAYS};
        const unsigned vals[3] = {samples, n.vertices, n.rays};
        block_stats<3>(rc.partials, which, vals);
    }
    // Some | None by pntaylor_make, the statements pntaylor_sample decides it with: 1 draw behind a sampler, none without
    static RL_DEV unsigned chain_skip(const DeviceScene& sc, bool has_max, float max_dist, V3 o, V3 d, float r_sel, float r_pos, V2 uv, const PnConst& pc) {
        const PnEmitter em = Pick::make(pc).on_ray(sc, o, d, has_max, max_dist, r_sel, r_pos, uv);
        PnTaylorDist ts;
        return pntaylor_make<STRATEGY>(sc.medium, pc, has_max, max_dist, o, d, em.p, em.n, &ts) ? 1u : 0u;
    }
};
template <int STRATEGY>
struct PnTaylor : PnTaylorBody<STRATEGY, PnPowerPick> {};

template <bool LDS_SCENE, int STRATEGY>
static void launch_pntaylor_one(bool chain, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PnConst& pc) {
    if (chain) hipLaunchKernelGGL((k_pn_chain<LDS_SCENE, PnTaylor<STRATEGY>>), grid, block, lds_bytes, st, rc, ds, stc, pc);
    else hipLaunchKernelGGL((k_pn_pixel<LDS_SCENE, PnTaylor<STRATEGY>>), grid, block, lds_bytes, st, rc, ds, stc, pc);
}
// chain = true: k_pn_chain, false: k_pn_pixel; strategy = rl_pn_taylor_strategy
template <bool LDS_SCENE>
static void launch_pntaylor_impl(bool chain, int strategy, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PnConst& pc) {
    switch (strategy) {
        case RL_PN_TAYLOR_EQ_PHASE: launch_pntaylor_one<LDS_SCENE, RL_PN_TAYLOR_EQ_PHASE>(chain, grid, block, lds_bytes, st, rc, ds, stc, pc); break;
        case RL_PN_TAYLOR_EQ_TR: launch_pntaylor_one<LDS_SCENE, RL_PN_TAYLOR_EQ_TR>(chain, grid, block, lds_bytes, st, rc, ds, stc, pc); break;
        case RL_PN_TAYLOR_EQ_CLAMPED_PHASE: launch_pntaylor_one<LDS_SCENE, RL_PN_TAYLOR_EQ_CLAMPED_PHASE>(chain, grid, block, lds_bytes, st, rc, ds, stc, pc); break;
        case RL_PN_TAYLOR_EQ_CLAMPED_TR: launch_pntaylor_one<LDS_SCENE, RL_PN_TAYLOR_EQ_CLAMPED_TR>(chain, grid, block, lds_bytes, st, rc, ds, stc, pc); break;
        case RL_PN_TAYLOR_PN_TR: launch_pntaylor_one<LDS_SCENE, RL_PN_TAYLOR_PN_TR>(chain, grid, block, lds_bytes, st, rc, ds, stc, pc); break;
        default: launch_pntaylor_one<LDS_SCENE, RL_PN_TAYLOR_PN_PHASE>(chain, grid, block, lds_bytes, st, rc, ds, stc, pc); break;
    }
}

}  // namespace rl
