// pnmis.hip.h — IntegratorPointNormal with use_mis (src/integrators/explicit/point_normal.rs:2605-2612): phase sampling and explicit light sampling combined
// with two or three distance samplers under the power heuristic.  Only the distance family of the strategy selects the function (the EX / PHASE bit is ignored):
//   PNMIS_TR       tr_*           compute_multiple_tr (:2095-2206)            transmittance distance; explicit + phase
//   PNMIS_EQ       eq_ex|phase    compute_multiple_equiangular (:1849-2091)   transmittance and equi-angular distances; explicit + phase from each
//   PNMIS_CLAMPED  eq_clamped_*   compute_multiple_strategy (:1560-1847)      the same two, and the clamped equi-angular sampler as a third (explicit only)
//   PNMIS_PN       pn_ex          the same with PointNormalSampling as the third
// Instantiated by pnmis_lds.hip (scene staged in LDS) and pnmis_stream.hip (BVH streamed from L2 / HBM).  The emitter sample, the three distance samplers and
// the sampler parking are pn.hip.h's, which this header includes and leaves as it is; new here are the pdf side of the samplers (EquiAngularSampling::
// {inside_bound, pdf} :135-175, PointNormalSampling::pdf :741-754, TransmittanceSampling::pdf :1118-1130), EmitterSampler::direct_pdf_ray / direct_pdf's
// non-ATS arm (emitter.rs:1537, 1574) through light_direct_pdf, and the four-pdf power heuristic.  Only the non-ATS arms are built.
//
// Draws per camera sample, in the order they are taken (after the 2 of the jitter; none with -z):
//   tr        1 distance, 4 emitter (next, next, next2d), 2 phase                                                  = 7
//   eq        1 transmittance, 4 emitter, 1 equi-angular, 2 phase                                                  = 8
//   clamped   4 emitter, 2 phase, 1 transmittance, 1 equi-angular, 1 more only when create_distance_sampling gave Some = 8 | 9
//   pn        the same                                                                                             = 8 | 9
// Every draw is unconditional and independent of a second ray, so pnmis_sample takes them all before its first second ray and parks the sampler there.
//
// Second rays per sample: tr 1 visibility + 1 phase; the others 2 visibility + 2 phase.  visible() is not called when n . (-d) <= 0 or when t_light is zero or
// not finite (the reference's || short-circuits).
//
// Kept as the reference has them: compute_multiple_strategy and compute_multiple_equiangular scale the flux by FRAC_1_PI whatever the emitter is, while
// compute_multiple_tr uses correct_flux(); a point light's zero normal makes every explicit technique zero (n . (-d) = 0 <= 0) and no phase ray hits a point
// light, so a point light adds nothing under MIS (it still takes its draws, and the equi-angular sampler is still built on its position).
//
// Where the reference panics, defined here once (tests/pnmis_restatement.py says the same):
//   (1) EquiAngularSampling::new asserts theta_a < theta_b (:42).  When it is the sampler built on the sampled light position, the sample takes its usual
//       draws, traces no second ray and adds zero.  When it is one built only to evaluate a pdf at a phase ray's hit (:1686, :1735), the contribution in which
//       it is built is zero.
//   (2) A transmittance sample that `exited` on an unbounded ray (:1093-1096): the sample takes its usual draws, traces no second ray and adds zero.
// The power heuristic is plain IEEE arithmetic, pdf_current^2 / (((0 + v0^2) + v1^2) + v2^2) + v3^2) in the order of the vec!: a 0 / 0 or inf / inf weight is
// NaN and flows into the colour through f32 * Color, which has no guard, as the reference's does.
//
// Drivers: pn.hip.h's, over the body PnMis<FAMILY> at the end of this header — k_pn_pixel<LDS_SCENE, PnMis<FAMILY>>, one lane per pixel with its samples in
// series, in its four sampler modes (per-sample fork; jump-ahead for tr and eq; the states the chain pass recorded for clamped and pn; the single-pass block
// walk); k_pn_chain<LDS_SCENE, PnMis<FAMILY>>, one lane per block, takes the jitter, the camera ray's closest hit and the four emitter draws, decides Some |
// None with pn_make_sampler — the statements pnmis_sample decides with — and skips 4 or 5 draws.  The order of a sample's four contributions is chosen for
// the registers: the two explicit ones first, each a finished value that its visibility ray keeps or drops, then the two phase ones, whose weights need the
// hit; the sum is taken in the reference's order.
#pragma once
#include "pn.hip.h"

namespace rl {

enum { PNMIS_TR = 0, PNMIS_EQ = 1, PNMIS_CLAMPED = 2, PNMIS_PN = 3 };

// EmitterSampler::random_sample_emitter_position (emitter.rs:1752-1762) without a correct_flux: flux = w / pdf_sel, pdf = sampled_pos.pdf * pdf_sel
struct PnMisEmitter { V3 p, n; Col flux; float pdf; bool surface; };
RL_DEV PnMisEmitter pnmis_sample_emitter(const DeviceScene& sc, float r_sel, float r_pos, V2 uv) {
    const unsigned id = cdf_sample(sc.emitters_cdf, sc.n_emitters + 1, r_sel);
    const float pdf_sel = sc.emitters_cdf[id + 1] - sc.emitters_cdf[id];
    const EmitterRecord em = sc.emitters[id];
    PnMisEmitter e;
    if (em.kind == EMITTER_MESH) {
        const MeshRecord& mr = sc.meshes[em.mesh];
        light_mesh_position(sc, mr, r_pos, uv, &e.p, &e.n, &e.flux);
        e.pdf = mr.inv_area * pdf_sel;                                      // PDF::Area(1 / cdf.total()) * pdf_sel
        e.surface = true;
    } else {                                                                // PointEmitter::sample_position (emitter.rs:217-229)
        e.p = mk3(em.v[0], em.v[1], em.v[2]); e.n = mk3(0.0f, 0.0f, 0.0f);
        e.flux = mkc(em.c[0], em.c[1], em.c[2]) * 4.0f * kPi;
        e.pdf = 1.0f * pdf_sel;                                             // PDF::Discrete(1.0) * pdf_sel
        e.surface = false;
    }
    e.flux = div_unguarded(e.flux, pdf_sel);
    return e;
}

// EquiAngularSampling::pdf (:168-175) of a sampler made by new (clamped = false: inside_bound is true)
RL_DEV float pnmis_pdf_equiangular(const PnDist& ds, float distance) {
    const float t = distance - ds.delta;
    return div_rn(ds.d_l, (ds.theta_b - ds.theta_a) * (ds.d_l * ds.d_l + t * t));
}
// EquiAngularSampling::inside_bound (:135-142) of a sampler made by new_clamping
RL_DEV bool pnmis_inside_bound(const PnDist& ds, float distance) {
    const float theta = pn_atan(div_rn(distance - ds.delta, ds.d_l));
    return theta >= ds.theta_a && theta <= ds.theta_b;
}
// the pdf of create_distance_sampling's sampler: EquiAngularSampling::pdf with clamped = true, or PointNormalSampling::pdf (:741-754)
template <int FAMILY>
RL_DEV float pnmis_pdf_third(const PnDist& ds, float distance) {
    if (!pnmis_inside_bound(ds, distance)) return 0.0f;
    if (FAMILY == PNMIS_CLAMPED) return pnmis_pdf_equiangular(ds, distance);
    const float t = distance - ds.delta;
    const float theta = pn_atan(div_rn(t, ds.d_l));
    const float pdf_angular = ds.a * dm::cosf_det(theta) + ds.b * dm::sinf_det(theta);
    const float jacobian = div_rn(ds.d_l, ds.d_l * ds.d_l + t * t);
    return fabsf(pdf_angular * jacobian);
}
// TransmittanceSampling::pdf (:1118-1130); the None arm is HomogenousVolume::pdf(ray, false) (volume.rs:143-150)
RL_DEV float pnmis_pdf_transmittance(const MediumRecord& m, bool has_max, float max_dist, float distance) {
    const Col sigma_t = mkc(m.sigma_t[0], m.sigma_t[1], m.sigma_t[2]);
    if (!has_max) {
        const Col tau = sigma_t * distance;
        return cavg(sigma_t * cexp(-tau));
    }
    const Col norm_c = cval(1.0f) - cexp((-sigma_t) * max_dist);
    return cavg((sigma_t / norm_c) * cexp((-sigma_t) * distance));
}
// pdf_current.powi(2) / pdfs.into_iter().map(|v| v.powi(2)).sum::<f32>(), pdfs[0] = pdf_current
RL_DEV float pnmis_power4(float v0, float v1, float v2, float v3) {
    const float sum = (((0.0f + v0 * v0) + v1 * v1) + v2 * v2) + v3 * v3;
    return div_rn(v0 * v0, sum);
}
template <int FAMILY> struct PnMisThird { static constexpr int strategy = FAMILY == PNMIS_PN ? RL_PN_PN_EX : RL_PN_EQ_CLAMPED_EX; };
// compute_pdf_other_clamped (:1574-1578): create_distance_sampling(ray, pos, n).map_or(0.0, |s| s.pdf(distance))
template <int FAMILY>
RL_DEV float pnmis_pdf_other_clamped(bool has_max, float max_dist, V3 o, V3 d, V3 pos, V3 n, float distance) {
    PnDist ds;
    if (!pn_make_sampler<PnMisThird<FAMILY>::strategy>(has_max, max_dist, o, d, pos, n, &ds)) return 0.0f;
    return pnmis_pdf_third<FAMILY>(ds, distance);
}

// An explicit contribution of compute_multiple_equiangular / compute_multiple_strategy (:2008-2046, :1759-1799) from the point p at the distance whose
// `transmittance / pdf` is trans: false = zero without a visibility ray; else *value is what the ray keeps or drops.  weight(pdf_ex, pdf_phase) gives w.
template <class W>
RL_DEV bool pnmis_explicit(const MediumRecord& m, V3 d, const PnMisEmitter& em, V3 p, Col trans, W&& weight, Col* value) {
    V3 d_light = em.p - p;
    const float t_light = length(d_light);
    if (t_light == 0.0f || !finite_f(t_light)) return false;
    d_light = d_light / t_light;
    const float cos_l = dot(em.n, -d_light);
    const float pdf_ex = div_rn(em.pdf * (t_light * t_light), cos_l);
    const Col flux = ((em.flux * kInvPi) * cos_l) / (t_light * t_light);
    if (cos_l <= 0.0f) return false;
    const Col light_trans = medium_transmittance(m, t_light);
    const float w = weight(pdf_ex, phase_pdf(m, -d, d_light));
    const Col sigma_s = mkc(m.sigma_s[0], m.sigma_s[1], m.sigma_s[2]);
    const Col v = flux * sigma_s * phase_eval(m, -d, d_light);
    *value = w * v * trans * light_trans;
    return true;
}

// A phase contribution (:1656-1703, :1916-1958, :2172-2203) from the point p: the ray along nd, the light it hits, its emission weighted by
// weight(pdf_ex, its.p, its.n_g, &w) — false: the contribution is zero (defined panic (1) at the hit).
template <class Stack, class W>
RL_DEV Col pnmis_phase(const DeviceScene& sc, const SceneRecs& recs, const Stack& stack, V3 p, V3 nd, Col trans, W&& weight, unsigned& n_rays) {
    Hit h2;
    n_rays++;
    if (!trace_closest(sc, recs, stack, p, nd, h2)) return czero();
    const SurfacePoint nx = fill_intersection(sc, h2.prim, h2.u, h2.v, p, nd, h2.t);
    const MeshRecord& nm = sc.meshes[nx.mesh];
    if (!(nm.flags & MESH_IS_LIGHT)) return czero();
    if (dot(nx.n_g, -nd) < 0.0f) return czero();
    const MediumRecord& m = sc.medium;
    const Col light_trans = medium_transmittance(m, length(nx.p - p));
    const float pdf_ex = light_direct_pdf<LIGHTS_AREA_ONLY>(sc, nm, 0, p, nx.p, nx.n_g, nd, false, nx.n_g);      // emitter.direct_pdf(ls) * self.pdf(emitter)
    float w;
    if (!weight(pdf_ex, nx.p, nx.n_g, &w)) return czero();
    const Col sigma_s = mkc(m.sigma_s[0], m.sigma_s[1], m.sigma_s[2]);
    const Col v = mesh_emit(sc, nm, nx.has_uv, nx.uv) * sigma_s * cone();      // sample_phase.weight is one for both phase functions
    return w * v * trans * light_trans;
}

// pnmis_sample<FAMILY> — compute_pixel with use_mis for one camera sample of pixel (px, py) on `rng`: the single body every driver calls.  `aa` is a run-time
// flag and park(rng) is called once, behind the sample's last draw, as in pn_sample.
template <int FAMILY, class Stack, class Park>
RL_DEV Col pnmis_sample(const DeviceScene& sc, const SceneRecs& recs, const Stack& stack, bool aa, unsigned px, unsigned py, Rng& rng, Park&& park,
                        unsigned& n_phase, unsigned& n_vis, unsigned& n_vertices) {
    float u = (float)px + 0.5f, v = (float)py + 0.5f;
    if (aa) { u = (float)px + rng_next_f32(rng); v = (float)py + rng_next_f32(rng); }
    const V3 o = mk3(sc.camera.position[0], sc.camera.position[1], sc.camera.position[2]);
    const V3 d = camera_direction(sc, u, v);
    Hit hit;
    const bool has_max = trace_closest(sc, recs, stack, o, d, hit);
    const float max_dist = hit.t;
    const MediumRecord& m = sc.medium;
    V3 nd; Col ph_weight; float pdf_phase;

    if (FAMILY == PNMIS_TR) {
        float t_cam, t_pdf;
        const bool ok = pn_sample_transmittance(m, has_max, max_dist, rng_next_f32(rng), &t_cam, &t_pdf);
        const float r_sel = rng_next_f32(rng), r_pos = rng_next_f32(rng);
        const V2 uv = smp_next2d(rng);
        const V2 s2 = smp_next2d(rng);
        park(rng);
        if (!ok) return czero();                                            // defined panic (2)
        n_vertices++;
        const V3 p = o + d * t_cam;
        const Col cam_trans = medium_transmittance(m, t_cam) / t_pdf;
        Col ex = czero();
        {
            const PnMisEmitter em = pnmis_sample_emitter(sc, r_sel, r_pos, uv);
            const Col flux0 = em.flux * (em.surface ? div_rn(1.0f, kPi) : div_rn(1.0f, 4.0f * kPi));      // flux * emitter.correct_flux()
            V3 d_light = em.p - p;
            const float t_light = length(d_light);
            if (!(t_light == 0.0f || !finite_f(t_light))) {
                d_light = d_light / t_light;
                const float cos_l = dot(em.n, -d_light);
                const float geom = div_rn(cos_l, t_light * t_light);
                const Col flux = flux0 * geom;
                if (!(cos_l <= 0.0f)) {
                    const Col sigma_s = mkc(m.sigma_s[0], m.sigma_s[1], m.sigma_s[2]);
                    const Col contrib = flux * sigma_s * phase_eval(m, -d, d_light);
                    const float pdf_ph = phase_pdf(m, -d, d_light);
                    const float pdf_ex = div_rn(em.pdf, geom);
                    const float w = div_rn(pdf_ex * pdf_ex, pdf_ph * pdf_ph + pdf_ex * pdf_ex);
                    const Col value = w * contrib * cam_trans * medium_transmittance(m, t_light);
                    n_vis++;
                    ex = shadow_visible(sc, recs, stack, p, em.p) ? value : czero();
                }
            }
        }
        phase_sample(m, -d, s2, &nd, &ph_weight, &pdf_phase);
        const Col ph = pnmis_phase(sc, recs, stack, p, nd, cam_trans, [&](float pdf_ex, V3, V3, float* w) {
            *w = div_rn(pdf_phase * pdf_phase, pdf_phase * pdf_phase + pdf_ex * pdf_ex);
            return true;
        }, n_phase);
        return ex + ph;
    }

    if (FAMILY == PNMIS_EQ) {
        float t_tr, pdf_tr, t_eq, pdf_eq;
        const bool ok_tr = pn_sample_transmittance(m, has_max, max_dist, rng_next_f32(rng), &t_tr, &pdf_tr);
        const float r_sel = rng_next_f32(rng), r_pos = rng_next_f32(rng);
        const V2 uv = smp_next2d(rng);
        const float xi_eq = rng_next_f32(rng);
        const V2 s2 = smp_next2d(rng);
        park(rng);
        const PnMisEmitter em = pnmis_sample_emitter(sc, r_sel, r_pos, uv);
        PnDist de;
        const bool ok_eq = pn_make_sampler<RL_PN_EQ_EX>(has_max, max_dist, o, d, em.p, em.n, &de);
        if (!ok_tr || !ok_eq) return czero();                               // the defined panics
        n_vertices++;
        pn_sample_equiangular(de, has_max, max_dist, xi_eq, &t_eq, &pdf_eq);
        const float pdf_eq_prime = pnmis_pdf_equiangular(de, t_tr);
        const float pdf_tr_prime = pnmis_pdf_transmittance(m, has_max, max_dist, t_eq);
        const V3 p_tr = o + d * t_tr, p_eq = o + d * t_eq;
        const Col trans_tr = medium_transmittance(m, t_tr) / pdf_tr, trans_eq = medium_transmittance(m, t_eq) / pdf_eq;
        Col ex_tr = czero(), ex_eq = czero(), value;
        if (pnmis_explicit(m, d, em, p_tr, trans_tr, [&](float pdf_ex, float pdf_ph) {
                return pnmis_power4(pdf_ex * pdf_tr, pdf_ph * pdf_tr, pdf_ph * pdf_eq_prime, pdf_ex * pdf_eq_prime); }, &value)) {
            n_vis++;
            ex_tr = shadow_visible(sc, recs, stack, p_tr, em.p) ? value : czero();
        }
        if (pnmis_explicit(m, d, em, p_eq, trans_eq, [&](float pdf_ex, float pdf_ph) {
                return pnmis_power4(pdf_ex * pdf_eq, pdf_ph * pdf_eq, pdf_ph * pdf_tr_prime, pdf_ex * pdf_tr_prime); }, &value)) {
            n_vis++;
            ex_eq = shadow_visible(sc, recs, stack, p_eq, em.p) ? value : czero();
        }
        phase_sample(m, -d, s2, &nd, &ph_weight, &pdf_phase);
        const Col ph_tr = pnmis_phase(sc, recs, stack, p_tr, nd, trans_tr, [&](float pdf_ex, V3, V3, float* w) {
            *w = pnmis_power4(pdf_phase * pdf_tr, pdf_ex * pdf_tr, pdf_phase * pdf_eq_prime, pdf_ex * pdf_eq_prime);
            return true;
        }, n_phase);
        const Col ph_eq = pnmis_phase(sc, recs, stack, p_eq, nd, trans_eq, [&](float pdf_ex, V3, V3, float* w) {
            *w = pnmis_power4(pdf_phase * pdf_eq, pdf_ex * pdf_eq, pdf_phase * pdf_tr_prime, pdf_ex * pdf_tr_prime);
            return true;
        }, n_phase);
        return ph_tr + ph_eq + ex_tr + ex_eq;
    }

    // compute_multiple_strategy
    {
        constexpr int THIRD = PnMisThird<FAMILY>::strategy;
        const float r_sel = rng_next_f32(rng), r_pos = rng_next_f32(rng);
        const V2 uv = smp_next2d(rng);
        const PnMisEmitter em = pnmis_sample_emitter(sc, r_sel, r_pos, uv);
        PnDist dc, de;
        const bool some = pn_make_sampler<THIRD>(has_max, max_dist, o, d, em.p, em.n, &dc);
        const bool ok_eq = pn_make_sampler<RL_PN_EQ_EX>(has_max, max_dist, o, d, em.p, em.n, &de);
        const V2 s2 = smp_next2d(rng);
        const float xi_tr = rng_next_f32(rng), xi_eq = rng_next_f32(rng);
        float xi_cl = 0.0f;
        if (some) { xi_cl = rng_next_f32(rng); n_vertices++; }
        park(rng);
        float t_tr, pdf_tr, t_eq, pdf_eq, t_cl = 0.0f, pdf_cl = 0.0f;
        const bool ok_tr = pn_sample_transmittance(m, has_max, max_dist, xi_tr, &t_tr, &pdf_tr);
        if (!ok_tr || !ok_eq) return czero();                               // the defined panics
        pn_sample_equiangular(de, has_max, max_dist, xi_eq, &t_eq, &pdf_eq);
        if (some) {
            if (FAMILY == PNMIS_PN) pn_sample_point_normal(dc, xi_cl, &t_cl, &pdf_cl);
            else pn_sample_equiangular(dc, has_max, max_dist, xi_cl, &t_cl, &pdf_cl);
        }
        const V3 p_tr = o + d * t_tr, p_eq = o + d * t_eq;
        const Col trans_tr = medium_transmittance(m, t_tr) / pdf_tr, trans_eq = medium_transmittance(m, t_eq) / pdf_eq;
        Col ex_tr = czero(), ex_cl = czero(), value;
        if (pnmis_explicit(m, d, em, p_tr, trans_tr, [&](float pdf_ex, float pdf_ph) {
                const float pdf_other = pnmis_pdf_equiangular(de, t_tr);
                const float pdf_other_clamped = some ? pnmis_pdf_third<FAMILY>(dc, t_tr) : 0.0f;
                return pnmis_power4(pdf_ex * pdf_tr, pdf_ph * pdf_tr, pdf_ph * pdf_other, pdf_ex * pdf_other_clamped); }, &value)) {
            n_vis++;
            ex_tr = shadow_visible(sc, recs, stack, p_tr, em.p) ? value : czero();
        }
        if (some && pdf_cl != 0.0f) {                                       // res_other_clamped (:1638-1653): None on a zero pdf, behind its draw
            const V3 p_cl = o + d * t_cl;
            const Col trans_cl = medium_transmittance(m, t_cl) / pdf_cl;
            if (pnmis_explicit(m, d, em, p_cl, trans_cl, [&](float pdf_ex, float pdf_ph) {
                    const float pdf_other = pnmis_pdf_equiangular(de, t_cl);
                    const float pdf_t = pnmis_pdf_transmittance(m, has_max, max_dist, t_cl);
                    return pnmis_power4(pdf_ex * pdf_cl, pdf_ph * pdf_other, pdf_ph * pdf_t, pdf_ex * pdf_t); }, &value)) {
                n_vis++;
                ex_cl = shadow_visible(sc, recs, stack, p_cl, em.p) ? value : czero();
            }
        }
        phase_sample(m, -d, s2, &nd, &ph_weight, &pdf_phase);
        const Col ph_tr = pnmis_phase(sc, recs, stack, p_tr, nd, trans_tr, [&](float pdf_ex, V3 ip, V3 in, float* w) {
            PnDist dh;
            if (!pn_make_sampler<RL_PN_EQ_EX>(has_max, max_dist, o, d, ip, in, &dh)) return false;      // defined panic (1) at the hit
            const float pdf_other = pnmis_pdf_equiangular(dh, t_tr);
            const float pdf_other_clamped = pnmis_pdf_other_clamped<FAMILY>(has_max, max_dist, o, d, ip, in, t_tr);
            *w = pnmis_power4(pdf_phase * pdf_tr, pdf_ex * pdf_tr, pdf_phase * pdf_other, pdf_ex * pdf_other_clamped);
            return true;
        }, n_phase);
        const Col ph_eq = pnmis_phase(sc, recs, stack, p_eq, nd, trans_eq, [&](float pdf_ex, V3 ip, V3 in, float* w) {
            PnDist dh;
            if (!pn_make_sampler<RL_PN_EQ_EX>(has_max, max_dist, o, d, ip, in, &dh)) return false;
            const float pdf_other = pnmis_pdf_equiangular(dh, t_eq);
            const float pdf_other_clamped = pnmis_pdf_other_clamped<FAMILY>(has_max, max_dist, o, d, ip, in, t_eq);
            const float pdf_t = pnmis_pdf_transmittance(m, has_max, max_dist, t_eq);
            *w = pnmis_power4(pdf_phase * pdf_other, pdf_ex * pdf_other_clamped, pdf_phase * pdf_t, pdf_ex * pdf_t);
            return true;
        }, n_phase);
        return ph_tr + ph_eq + ex_tr + ex_cl;
    }
}

// PnMis<FAMILY> — pnmis_sample as a body of pn.hip.h's drivers (PnPlain<STRATEGY> is the other one).
template <int FAMILY>
struct PnMis {
    // waves per SIMD k_pn_pixel is compiled for (the resource rows record what each family reached)
    static constexpr int kWaves = FAMILY == PNMIS_TR ? 4 : 3;
    static constexpr unsigned kEmitterDraws = 4;        // the power pick's, which k_pn_chain takes before chain_skip
    struct Counts { unsigned phase = 0, vis = 0, vertices = 0; };
    template <class Stack, class Park>
    static RL_DEV Col sample(const DeviceScene& sc, const SceneRecs& recs, const Stack& stack, bool aa, unsigned px, unsigned py, Rng& rng, Park&& park, Counts& n, const PnConst&) {
        return pnmis_sample<FAMILY>(sc, recs, stack, aa, px, py, rng, park, n.phase, n.vis, n.vertices);
    }
    // four rows; the host derives the five counters from them (pnmis_render.hip.h): a sample's draws follow from its family and from whether its third
    // sampler was Some (STAT_VERTICES for clamped and pn; for tr and eq that row counts the samples no defined panic ended)
    static RL_DEV void stats(const RenderConst& rc, unsigned samples, const Counts& n) {
        const int which[4] = {STAT_SAMPLES, STAT_VERTICES, STAT_EXT_RAYS, STAT_SHADOW_RAYS};
        const unsigned vals[4] = {samples, n.vertices, n.phase, n.vis};
        block_stats<4>(rc.partials, which, vals);
    }
    // clamped and pn: Some | None of the third sampler by pn_make_sampler, the statements pnmis_sample decides it with; 4 draws, and one more behind a sampler
    static RL_DEV unsigned chain_skip(const DeviceScene& sc, bool has_max, float max_dist, V3 o, V3 d, float r_sel, float r_pos, V2 uv, const PnConst&) {
        const PnMisEmitter em = pnmis_sample_emitter(sc, r_sel, r_pos, uv);
        PnDist ds;
        return pn_make_sampler<PnMisThird<FAMILY>::strategy>(has_max, max_dist, o, d, em.p, em.n, &ds) ? 5u : 4u;
    }
};

// chain = true: k_pn_chain (clamped and pn only; any other family launches nothing), false: k_pn_pixel
template <bool LDS_SCENE>
static void launch_pnmis_impl(bool chain, int family, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PnConst& pc) {
    if (chain) {
        if (family == PNMIS_CLAMPED) hipLaunchKernelGGL((k_pn_chain<LDS_SCENE, PnMis<PNMIS_CLAMPED>>), grid, block, lds_bytes, st, rc, ds, stc, pc);
        else if (family == PNMIS_PN) hipLaunchKernelGGL((k_pn_chain<LDS_SCENE, PnMis<PNMIS_PN>>), grid, block, lds_bytes, st, rc, ds, stc, pc);
        return;
    }
    if (family == PNMIS_TR) hipLaunchKernelGGL((k_pn_pixel<LDS_SCENE, PnMis<PNMIS_TR>>), grid, block, lds_bytes, st, rc, ds, stc, pc);
    else if (family == PNMIS_EQ) hipLaunchKernelGGL((k_pn_pixel<LDS_SCENE, PnMis<PNMIS_EQ>>), grid, block, lds_bytes, st, rc, ds, stc, pc);
    else if (family == PNMIS_CLAMPED) hipLaunchKernelGGL((k_pn_pixel<LDS_SCENE, PnMis<PNMIS_CLAMPED>>), grid, block, lds_bytes, st, rc, ds, stc, pc);
    else hipLaunchKernelGGL((k_pn_pixel<LDS_SCENE, PnMis<PNMIS_PN>>), grid, block, lds_bytes, st, rc, ds, stc, pc);
}

}  // namespace rl
