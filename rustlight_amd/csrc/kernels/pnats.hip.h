// pnats.hip.h — IntegratorPointNormal over the light tree (`-x ats`, CLI `point-normal-ats`): the emitter pick PnAtsPick for the sample bodies of pn.hip.h
// (the seven plain strategies) and pntaylor.hip.h (the six Taylor strategies).  The bodies are theirs; only where the emitter position comes from differs.
// Instantiated by pnats_lds.hip and pnats_stream.hip as k_pn_pixel / k_pn_chain over PnAts<FAMILY, STRATEGY>.
//
// on_ray — fix_random_sample_emitter's ATS arm (point_normal.rs:1217-1228), every strategy but the two tr_*: sampler.next(), sampler.next2d() — three draws
// where the power pick takes four —, EmitterSampler::random_sample_emitter_position_ray (emitter.rs:1732-1750): LightSamplerATS::sample (:1361-1399) from the
// root with LightBounds::importance_ray(ray, max_dist) (:975-1032), then sample_position_tri(primitive, uv) (:690-698), pdf = pdf_tri * pdf_sel,
// flux = (emit(uv) * PI / pdf_tri) / pdf_sel * correct_flux().
// at_point — compute_single_tr's ATS arm (:2237-2243), tr_ex: behind the distance draw, random_sample_emitter_position_point(&p, None, next, next2d)
// (emitter.rs:1649-1667): shading.hip.h's ats_sample with has_n = false at the scattering point, then the same sample_position_tri.
// tr_phase takes no emitter sample: PnAts<0, RL_PN_TR_PHASE> is PnPlain<RL_PN_TR_PHASE>'s code.
//
// Draws per camera sample behind the jitter:   tr_ex 1 + 3 = 4 | tr_phase 3 | eq_ex 3 + 1 = 4 | eq_phase 3 + 1 + 2 = 6 | eq_clamped_ex, pn_ex 3 | 4 |
// eq_clamped_phase 3 | 6 | the Taylor names 3 | 4.  The constant ones enter the block's stream by rng_advance, the others take the chain pass, where
// k_pn_chain takes Body::kEmitterDraws = 3 draws and chain_skip decides Some | None behind the same walk.
//
// importance_ray, statement by statement: closest_squared_distance_ray_point (math.rs:5-31), d = sqrt(max(d2, EPSILON_ATS)); v0 = normalize(o - pc),
// v1 = normalize(o + d * max_dist - pc), or -d on a miss; o0 = v0, up = normalize(v0 x v1), o1 = up x v0; cos_phi_0 = dot_o0 / sqrt(max(dot_o0^2 + dot_o1^2, 0));
// cos_theta_min = max(v0 . w, v1 . w) when dot_o1 < 0 or v0 . v1 < cos_phi_0, else (o0 cos_phi_0 + o1 sin_phi_0) . w; theta_min = acos_fast (math.rs:74-88, a
// cubic times sqrt(1 - |x|), not acos); theta_u = acos_fast of subtended_directions at the closest point (ats_cos_subtended);
// theta_p = max(theta_min - theta_o - theta_u, 0); zero at theta_p >= theta_e, else max(phi * cos(theta_p) / d, 0) with cos = cosf_det.
// theta_o and theta_e are read as angles: LightNode holds their cosines only, so the two angles of every node come in a side array (PnConst::ats_angles, the
// host tree's stored safe_acos results, not an acos of the stored cosine).
//
// Where the reference panics, defined here once (the restatement tests/pnats_restatement.py says the same):
//   (1) assert!(cos_phi_0.is_finite()) (emitter.rs:1008) fires when the cluster's centre lies on the ray's line (v0 x v1 = 0: `up` is NaN, f32::max drops the
//       NaN, the divisor is zero) or its axis is normal to the plane of v0 and v1 (0 / 0).  Such a node has importance 0.
//   (2) LightSamplerATS::new asserts that every emitter is a surface: the host refuses a scene with another kind of emitter before any kernel.
// Kept as the reference has it: two children of importance 0 give prob_left = 0.5; the warning "Wrong sign" is not an event; NaN goes through acos_fast and
// the comparisons literally (f32::max ignores it); Color / f32 guards its divisor.
#pragma once
#include "pntaylor.hip.h"

namespace rl {

enum { PNATS_PLAIN = 0, PNATS_TAYLOR = 1 };     // rl_pn_ats_family

// math::acos_fast (math.rs:74-88)
RL_DEV float pnats_acos_fast(float x) {
    const float x1 = fabsf(x);
    const float x2 = x1 * x1;
    const float x3 = x2 * x1;
    float s = -0.2121144f * x1 + kPi2;
    s = 0.0742610f * x2 + s;
    s = -0.0187293f * x3 + s;
    s = sqrt_rn(1.0f - x1) * s;
    return x >= 0.0f ? s : kPi - s;
}

// LightBounds::importance_ray (emitter.rs:975-1032); theta_o, theta_e: the node's angles
RL_DEV float pnats_importance_ray(const LightNode& nd, float theta_o, float theta_e, V3 o, V3 d, bool has_max, float max_dist) {
    const V3 bmin = mk3(nd.bmin[0], nd.bmin[1], nd.bmin[2]), bmax = mk3(nd.bmax[0], nd.bmax[1], nd.bmax[2]);
    const V3 w = mk3(nd.axis[0], nd.axis[1], nd.axis[2]);
    const V3 pc = (bmax - bmin) * 0.5f + bmin;
    // closest_squared_distance_ray_point (math.rs:5-31)
    float t = dot(d, pc - o);
    t = t > 0.0f ? ((has_max && !(max_dist >= t)) ? max_dist : t) : 0.0f;
    const V3 closest = o + d * t;
    const float dist = sqrt_rn(rmax(length2(pc - closest), 0.0001f));
    const V3 v0 = normalize(o - pc);
    const V3 v1 = has_max ? normalize((o + d * max_dist) - pc) : -d;
    const V3 up = normalize(cross(v0, v1));
    const V3 o1 = cross(up, v0);
    const float dot_o0 = dot(v0, w);
    const float dot_o1 = dot(o1, w);
    const float length_1 = sqrt_rn(rmax(dot_o0 * dot_o0 + dot_o1 * dot_o1, 0.0f));
    const float cos_phi_0 = div_rn(dot_o0, length_1);
    if (!finite_f(cos_phi_0)) return 0.0f;                                  // defined panic (1)
    float cos_theta_min;
    if (dot_o1 < 0.0f || dot(v0, v1) < cos_phi_0) cos_theta_min = rmax(dot(v0, w), dot(v1, w));
    else {
        const float sin_phi_0 = sqrt_rn(1.0f - cos_phi_0 * cos_phi_0);
        cos_theta_min = dot(v0 * cos_phi_0 + o1 * sin_phi_0, w);
    }
    const float theta_min = pnats_acos_fast(cos_theta_min);
    const float theta_u = pnats_acos_fast(ats_cos_subtended(bmin, bmax, closest));
    const float theta_p = rmax(theta_min - theta_o - theta_u, 0.0f);
    if (theta_p >= theta_e) return 0.0f;
    return rmax(div_rn(nd.phi * dm::cosf_det(theta_p), dist), 0.0f);
}

// LightSamplerATS::sample (emitter.rs:1361-1399) with importance_ray: a loop down one root-to-leaf path, two child importances per level, no stack.
// Returns the light proxy, *pdf_sel its probability.
RL_DEV int pnats_sample_ray(const DeviceScene& sc, const float* angles, float r, V3 o, V3 d, bool has_max, float max_dist, float* pdf_sel) {
    float pdf = 1.0f;
    int ni = sc.ats_root;
    for (;;) {
        const int left = sc.ats_nodes[ni].left, right = sc.ats_nodes[ni].right;
        if (left < 0 && right < 0) { *pdf_sel = pdf; return sc.ats_nodes[ni].light; }
        const float il = pnats_importance_ray(sc.ats_nodes[left], angles[2 * left], angles[2 * left + 1], o, d, has_max, max_dist);
        const float ir = pnats_importance_ray(sc.ats_nodes[right], angles[2 * right], angles[2 * right + 1], o, d, has_max, max_dist);
        const float pl = (il == 0.0f && ir == 0.0f) ? 0.5f : div_rn(il, il + ir);
        if (r < pl) { r = div_rn(r, pl); ni = left; pdf = pdf * pl; }
        else { r = div_rn(r - pl, 1.0f - pl); ni = right; pdf = pdf * (1.0f - pl); }
    }
}

// Mesh::sample_position_tri (emitter.rs:690-698) over Mesh::sample_tri (geometry.rs:261-338) of light proxy `li`, then w / pdf_sel and * correct_flux():
// light.hip.h's light_mesh_position for a given triangle, with pdf = 1 / area_tri (pdf_tri, geometry.rs:226-234).  Written here and not split out of
// light_mesh_position: that function is inlined into the light, VPL, beam and plane generation kernels, whose code objects this change leaves alone.
RL_DEV PnEmitter pnats_emitter(const DeviceScene& sc, int li, float pdf_sel, V2 uv) {
    const MeshRecord mr = sc.meshes[sc.ats_light_mesh[li]];
    const unsigned gtri = mr.tri_base + (unsigned)sc.ats_light_prim[li];
    const unsigned i0 = sc.tri_indices[3 * gtri], i1 = sc.tri_indices[3 * gtri + 1], i2 = sc.tri_indices[3 * gtri + 2];
    const V3 v0 = mk3(sc.positions[3 * i0], sc.positions[3 * i0 + 1], sc.positions[3 * i0 + 2]);
    const V3 v1 = mk3(sc.positions[3 * i1], sc.positions[3 * i1 + 1], sc.positions[3 * i1 + 2]);
    const V3 v2 = mk3(sc.positions[3 * i2], sc.positions[3 * i2 + 1], sc.positions[3 * i2 + 2]);
    const V2 b = uniform_sample_triangle(uv);
    const float w2 = 1.0f - b.x - b.y;
    PnEmitter e;
    e.p = v0 * b.x + v1 * b.y + v2 * w2;
    V3 n_g = normalize(cross(v2 - v0, v1 - v0));
    if (mr.flags & MESH_HAS_NORMALS) {
        const V3 n0 = mk3(sc.normals[3 * i0], sc.normals[3 * i0 + 1], sc.normals[3 * i0 + 2]);
        const V3 n1 = mk3(sc.normals[3 * i1], sc.normals[3 * i1 + 1], sc.normals[3 * i1 + 2]);
        const V3 n2 = mk3(sc.normals[3 * i2], sc.normals[3 * i2 + 1], sc.normals[3 * i2 + 2]);
        V3 n = n0 * b.x + n1 * b.y + n2 * w2;
        const float nl = length2(n);
        if (nl == 0.0f) n = n_g;
        else if (nl != 1.0f) n = n / sqrt_rn(nl);
        if (dot(n_g, n) < 0.0f) n_g = -n_g;
    }
    e.n = n_g;
    Col emit;
    if (__builtin_expect(mr.emission_type == 0, 1)) emit = mkc(mr.emission[0], mr.emission[1], mr.emission[2]);
    else emit = mesh_emit_sampled(sc.bitmaps, sc.bitmap_texels, sc.uvs, mr.emission_type, mr.emission_scale, mr.emission_bitmap, (mr.flags & MESH_HAS_UV) != 0, i0, i1, i2, b.x, b.y, w2);
    const float pdf_tri = div_rn(1.0f, length(cross(v1 - v0, v2 - v0)) * 0.5f);
    e.flux = ((emit * kPi) / pdf_tri) / pdf_sel;
    e.flux = e.flux * div_rn(1.0f, kPi);                                   // correct_flux (emitter.rs:601-603)
    e.surface = true;
    return e;
}

// The light tree's emitter pick (pn.hip.h's PnPowerPick is the other one): next, next2d
struct PnAtsPick {
    static constexpr unsigned kDraws = 3;
    const float* angles;
    static RL_DEV PnAtsPick make(const PnConst& pc) { return {pc.ats_angles}; }
    RL_DEV PnEmitter on_ray(const DeviceScene& sc, V3 o, V3 d, bool has_max, float max_dist, float r_sel, float, V2 uv) const {
        float pdf_sel;
        const int li = pnats_sample_ray(sc, angles, r_sel, o, d, has_max, max_dist, &pdf_sel);
        return pnats_emitter(sc, li, pdf_sel, uv);
    }
    RL_DEV PnEmitter at_point(const DeviceScene& sc, V3 p, float r_sel, float, V2 uv) const {
        float pdf_sel;
        const int li = ats_sample(sc, r_sel, p, false, mk3(0.0f, 0.0f, 0.0f), &pdf_sel);
        return pnats_emitter(sc, li, pdf_sel, uv);
    }
};

// waves per SIMD k_pn_pixel is compiled for (profiles/pnats_note.md records what the compiler reported at four): the plain bodies keep four; of the Taylor
// bodies the four eq / eq_clamped names spill 1 to 3 VGPRs at four behind the walk's three draws (r_sel and uv are live across it) and are compiled for
// three, pn_tr_taylor_ex fits four, pn_phase_taylor_ex sits at three as it does over the power pick
constexpr int pnats_waves(int family, int strategy) { return family == PNATS_TAYLOR ? (strategy == RL_PN_TAYLOR_PN_TR ? kPnWaves : 3) : kPnWaves; }
// PnAts<FAMILY, STRATEGY> — the plain body (FAMILY = PNATS_PLAIN, STRATEGY an rl_pn_strategy) or the Taylor body (PNATS_TAYLOR, an rl_pn_taylor_strategy) over
// the light tree's pick
template <int FAMILY, int STRATEGY>
struct PnAts : std::conditional_t<FAMILY == PNATS_TAYLOR, PnTaylorBody<STRATEGY, PnAtsPick, pnats_waves(FAMILY, STRATEGY)>,
                                  PnPlainBody<STRATEGY, PnAtsPick, pnats_waves(FAMILY, STRATEGY)>> {};

template <bool LDS_SCENE, int FAMILY, int STRATEGY>
static void launch_pnats_one(bool chain, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PnConst& pc) {
    // the chain pass: the Taylor names and the three plain strategies whose sampler can be None; any other strategy launches nothing
    constexpr bool has_chain = FAMILY == PNATS_TAYLOR || STRATEGY == RL_PN_EQ_CLAMPED_EX || STRATEGY == RL_PN_EQ_CLAMPED_PHASE || STRATEGY == RL_PN_PN_EX;
    if (!chain) hipLaunchKernelGGL((k_pn_pixel<LDS_SCENE, PnAts<FAMILY, STRATEGY>>), grid, block, lds_bytes, st, rc, ds, stc, pc);
    else if constexpr (has_chain) hipLaunchKernelGGL((k_pn_chain<LDS_SCENE, PnAts<FAMILY, STRATEGY>>), grid, block, lds_bytes, st, rc, ds, stc, pc);
}
// chain = true: k_pn_chain, false: k_pn_pixel; selector = 8 * rl_pn_ats_family + the strategy within the family
template <bool LDS_SCENE>
static void launch_pnats_impl(bool chain, int selector, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PnConst& pc) {
    const int strategy = selector & 7;
    if ((selector >> 3) == PNATS_TAYLOR) {
        switch (strategy) {
            case RL_PN_TAYLOR_EQ_PHASE: launch_pnats_one<LDS_SCENE, PNATS_TAYLOR, RL_PN_TAYLOR_EQ_PHASE>(chain, grid, block, lds_bytes, st, rc, ds, stc, pc); break;
            case RL_PN_TAYLOR_EQ_TR: launch_pnats_one<LDS_SCENE, PNATS_TAYLOR, RL_PN_TAYLOR_EQ_TR>(chain, grid, block, lds_bytes, st, rc, ds, stc, pc); break;
            case RL_PN_TAYLOR_EQ_CLAMPED_PHASE: launch_pnats_one<LDS_SCENE, PNATS_TAYLOR, RL_PN_TAYLOR_EQ_CLAMPED_PHASE>(chain, grid, block, lds_bytes, st, rc, ds, stc, pc); break;
            case RL_PN_TAYLOR_EQ_CLAMPED_TR: launch_pnats_one<LDS_SCENE, PNATS_TAYLOR, RL_PN_TAYLOR_EQ_CLAMPED_TR>(chain, grid, block, lds_bytes, st, rc, ds, stc, pc); break;
            case RL_PN_TAYLOR_PN_TR: launch_pnats_one<LDS_SCENE, PNATS_TAYLOR, RL_PN_TAYLOR_PN_TR>(chain, grid, block, lds_bytes, st, rc, ds, stc, pc); break;
            default: launch_pnats_one<LDS_SCENE, PNATS_TAYLOR, RL_PN_TAYLOR_PN_PHASE>(chain, grid, block, lds_bytes, st, rc, ds, stc, pc); break;
        }
        return;
    }
    with_pn_strategy(strategy, [&](auto s) { launch_pnats_one<LDS_SCENE, PNATS_PLAIN, decltype(s)::value>(chain, grid, block, lds_bytes, st, rc, ds, stc, pc); });
}

}  // namespace rl
