// plane.hip.h — IntegratorSinglePlane (src/integrators/explicit/plane_single.rs): single scattering from rectangular area lights estimated with photon
// planes.  The device pieces every plane integrator shares come first — SinglePhotonPlane::new, intersection, light_position, contrib and the weights of the
// seven strategies —, then the gather kernel, instantiated by plane_lds.hip (scene staged in LDS) and plane_stream.hip (BVH streamed from L2 / HBM).  The
// generation kernels (k_plane_generate, k_plane_generate_lanes, plane_generate.hip) and the uncorrelated integrator (k_uplane, uplane.hip.h) are built from the same
// pieces.
//
// The gather is beam_gather (gather.hip.h) over the leaf below, through the plane tree (host/planetree.cpp).  Plane: 4 float4 = o, length0 | d0, length1 |
// d1, type + 4 * id_emitter | weight, 0; the weight is loaded for visible planes only.
#pragma once
#include "gather.hip.h"

namespace rl {

struct Plane { V3 o, d0, d1; float l0, l1; Col weight; unsigned type; };
struct PlaneIts { float t_cam, t0, t1; };

RL_DEV V3 pl3(const float* p) { return mk3(p[0], p[1], p[2]); }

// SinglePhotonPlane::new (plane_single.rs:177-277).  f32::max / min ignore a NaN operand: rmax / rmin
RL_DEV Plane plane_new(unsigned type, const PlaneLight& l, V3 d, V2 sample, float sample_alpha, float t_sampled, Col sigma_s) {
    const V3 lo = pl3(l.o), lu = pl3(l.u), lv = pl3(l.v);
    const Col emission = mkc(l.emission[0], l.emission[1], l.emission[2]);
    Plane p;
    p.type = type;
    if (type == RL_PLANE_UV) {
        p.o = lo + d * t_sampled;
        p.d0 = lu; p.d1 = lv; p.l0 = l.u_l; p.l1 = l.v_l;
        p.weight = (kPi * emission) / sigma_s;                    // sigma_s cancels the sampled distance's
    } else if (type == RL_PLANE_VT) {
        p.o = lo + lu * l.u_l * sample.x;
        p.d0 = lv; p.d1 = d; p.l0 = l.v_l; p.l1 = t_sampled;
        p.weight = (kPi * l.u_l) * emission;
    } else if (type == RL_PLANE_UT) {
        p.o = lo + lv * l.v_l * sample.y;
        p.d0 = lu; p.d1 = d; p.l0 = l.u_l; p.l1 = t_sampled;
        p.weight = (kPi * l.v_l) * emission;
    } else {                                                      // UAlphaT
        const float alpha = kPi * sample_alpha;
        const float ox = sample.x * l.u_l, oy = sample.y * l.v_l;
        const float dx = m_cosf(alpha), dy = m_sinf(alpha);
        float px[2], py[2];
#pragma unroll
        for (int k = 0; k < 2; k++) {                             // plane2d_its(d_plane, o_plane), plane2d_its(-d_plane, o_plane)
            const float ddx = k ? -dx : dx, ddy = k ? -dy : dy;
            const float t0x = div_rn(-ox, ddx), t0y = div_rn(-oy, ddy);
            const float t1x = div_rn(l.u_l - ox, ddx), t1y = div_rn(l.v_l - oy, ddy);
            const float t = rmin(rmax(t0x, t1x), rmax(t0y, t1y));
            px[k] = ox + ddx * t; py[k] = oy + ddy * t;
        }
        const V3 p1 = lo + px[0] * lu + py[0] * lv;
        const V3 p2 = lo + px[1] * lu + py[1] * lv;
        V3 u_plane = p2 - p1;
        const float len = length(u_plane);
        u_plane = u_plane / len;
        p.o = p1; p.d0 = u_plane; p.d1 = d; p.l0 = len; p.l1 = t_sampled;
        p.weight = ((kPi * emission) * (l.u_l * l.v_l)) / len;
    }
    return p;
}

// generate_plane (plane_single.rs:326-361, uncorrelated_plane_single.rs:44-79) for a plane of type `type` on `light`: cosine_sample_hemisphere(next2d()), next() for the
// medium's distance (HomogenousVolume::sample on Ray::new(light.o, d), volume.rs:95-135: continued_t, the distance sampled whatever the ray's tfar is), next2d() for
// `sample`, next() for alpha, SinglePhotonPlane::new.  false, after the direction's 2 draws alone, when its z is 0: the reference draws the direction again, and so
// does the caller — by calling again (the serial walks) or by giving the stream up (k_plane_generate_lanes).
RL_DEV bool plane_sample(Rng& rng, unsigned type, const PlaneLight& light, Col sigma_t, Col sigma_s, Plane* p, V2* sample) {
    const V3 d_out = cosine_sample_hemisphere(smp_next2d(rng));
    if (d_out.z == 0.0f) return false;
    const V3 d = to_world(make_frame(pl3(light.n)), d_out);
    float xi = rng_next_f32(rng);
    const float u3 = xi * 3.0f;
    const int component = u3 != u3 ? 0 : (u3 <= 0.0f ? 0 : (u3 >= 255.0f ? 255 : (int)u3));   // `as u8`
    xi = xi * 3.0f - (float)component;
    const float t_sampled = div_rn(-m_logf(1.0f - xi), cget(sigma_t, component));
    *sample = smp_next2d(rng);
    const float alpha = rng_next_f32(rng);
    *p = plane_new(type, light, d, *sample, alpha, t_sampled, sigma_s);
    return true;
}

// BVHElement::intersection (plane_single.rs:121-160): the triangle test without its u + v <= 1.  The comparisons are the reference's, so a NaN passes where it
// passes there.
RL_DEV bool plane_intersect(V3 po, V3 d0, V3 d1, float l0, float l1, V3 ro, V3 rd, float tnear, float tfar, PlaneIts* its) {
    const V3 e0 = d0 * l0, e1 = d1 * l1;
    const V3 p = cross(rd, e1);
    const float det = dot(e0, p);
    if (fabsf(det) < 1e-5f) return false;
    const float inv_det = div_rn(1.0f, det);
    const V3 t = ro - po;
    const float t0 = dot(t, p) * inv_det;
    if (t0 < 0.0f || t0 > 1.0f) return false;
    const V3 q = cross(t, e0);
    const float t1 = dot(rd, q) * inv_det;
    if (t1 < 0.0f || t1 > 1.0f) return false;
    const float t_cam = dot(e1, q) * inv_det;
    if (t_cam <= tnear || t_cam >= tfar) return false;
    its->t_cam = t_cam; its->t1 = t1 * l1; its->t0 = t0 * l0;      // scaled to distances
    return true;
}
// SinglePhotonPlane::light_position (163-172)
RL_DEV V3 plane_light_position(unsigned type, V3 po, V3 d0, const PlaneLight& l, const PlaneIts& its) {
    if (type == RL_PLANE_UV) return pl3(l.o) + pl3(l.u) * its.t0 + pl3(l.v) * its.t1;
    return po + d0 * its.t0;
}
// SinglePhotonPlane::contrib (173-176): weight / |d1 x d0 . d| (Color / f32: black for a zero or non-finite jacobian)
RL_DEV Col plane_contrib(Col weight, V3 d0, V3 d1, V3 d) { return weight / fabsf(dot(cross(d1, d0), d)); }
// DiscreteMIS (493-560): the balance heuristic over the UV, UT and VT planes re-made through the gathered point
RL_DEV float plane_discrete_mis(unsigned type, const PlaneLight& l, Col sigma_s, V3 p_hit, V3 p_light, V3 rd) {
    V3 d = p_hit - p_light;
    const float t_sampled = length(d);
    d = d / t_sampled;
    const V3 lu = pl3(l.u), lv = pl3(l.v);
    const Col emission = mkc(l.emission[0], l.emission[1], l.emission[2]);
    const float c_uv = cavg(plane_contrib((kPi * emission) / sigma_s, lu, lv, rd));
    const float c_ut = cavg(plane_contrib((kPi * l.v_l) * emission, lu, d, rd));
    const float c_vt = cavg(plane_contrib((kPi * l.u_l) * emission, lv, d, rd));
    const float own = type == RL_PLANE_UV ? c_uv : (type == RL_PLANE_UT ? c_ut : c_vt);
    const float a = (c_uv != 0.0f && finite_f(c_uv)) ? div_rn(1.0f, c_uv) : 0.0f;
    const float b = (c_ut != 0.0f && finite_f(c_ut)) ? div_rn(1.0f, c_ut) : 0.0f;
    const float c = (c_vt != 0.0f && finite_f(c_vt)) ? div_rn(1.0f, c_vt) : 0.0f;
    const float w = div_rn(div_rn(1.0f, own), (a + b) + c);
    return finite_f(w) ? w : 0.0f;
}
// ContinousMIS (567-585): 1 / ((2 / PI) * sqrt((u x d1 . d)^2 + (v x d1 . d)^2))
RL_DEV float plane_w_cmis(const PlaneLight& l, V3 d1, V3 rd) {
    const float a = dot(cross(pl3(l.u), d1), rd), b = dot(cross(pl3(l.v), d1), rd);
    return div_rn(1.0f, div_rn(2.0f, kPi) * sqrt_rn(a * a + b * b));
}

// MODE: PLAIN = a run-time w (1 for UV / VT / UT / UAlpha, 1 / 3 for Average: 1.0 * rho is exact), DISCRETE_MIS, CMIS
// What a plane the camera ray meets adds (plane_single.rs:463-596, uncorrelated_plane_single.rs:185-292): the point on the light, one visibility ray — false when it
// is blocked —, then cs += w * rho * transmittance * sigma_s * flux * n_lights * inv_gen.  weight() is asked for visible planes only.
template <int MODE, class STACK, class WEIGHT>
RL_DEV bool plane_contribution(unsigned type, V3 po, V3 d0, V3 d1, const PlaneLight& light, const PlaneIts& its, V3 cam, V3 rd, const DeviceScene& sc, const SceneRecs& recs,
                               const STACK& stack, float w, float n_lights_f, float inv_gen, WEIGHT&& weight_of, Col& cs) {
    const V3 p_hit = cam + rd * its.t_cam;
    const V3 p_light = plane_light_position(type, po, d0, light, its);
    if (!shadow_visible(sc, recs, stack, p_hit, p_light)) return false;
    const Col weight = weight_of();
    const Col trans = medium_transmittance(sc.medium, its.t_cam);
    const Col sigma_s = mkc(sc.medium.sigma_s[0], sc.medium.sigma_s[1], sc.medium.sigma_s[2]);
    const Col rho = cval(div_rn(1.0f, kPi * 4.0f));                 // PhaseFunction::Isotropic(), whatever the medium's phase function is (plane_single.rs:440)
    if (MODE == PLANE_MODE_DISCRETE_MIS) w = plane_discrete_mis(type, light, sigma_s, p_hit, p_light, rd);
    Col flux;
    if (MODE == PLANE_MODE_CMIS) flux = plane_w_cmis(light, d1, rd) * weight;
    else flux = plane_contrib(weight, d0, d1, rd);
    // c += w * rho * transmittance * sigma_s * flux * (emitters.len() as f32) * (1.0 / number_plane_gen as f32)
    cs = cs + (((((w * rho) * trans) * sigma_s) * flux) * n_lights_f) * inv_gen;
    return true;
}

template <int MODE>
struct PlaneLeaf {
    PlaneConst c;
    static constexpr int kCounters = 2;                                     // planes intersected, of those visible
    static constexpr int kLo[2] = {STAT_PLANE_ISECT, STAT_PLANE_VISIBLE}, kHi[2] = {STAT_PLANE_ISECT_HI, STAT_PLANE_VISIBLE_HI};
    template <class STACK>
    RL_DEV void element(unsigned idx, V3 cam, V3 rd, float tfar, const DeviceScene& sc, const SceneRecs& recs, const STACK& stack, Col& cs, unsigned long long (&n)[2]) const {
        const float4* pl = c.planes + 4u * (size_t)idx;
        const float4 q0 = pl[0], q1 = pl[1], q2 = pl[2];
        const V3 po = mk3(q0.x, q0.y, q0.z), d0 = mk3(q1.x, q1.y, q1.z), d1 = mk3(q2.x, q2.y, q2.z);
        PlaneIts its;
        if (!plane_intersect(po, d0, d1, q0.w, q1.w, cam, rd, kEps, tfar, &its)) return;
        n[0]++;
        const unsigned tb = __float_as_uint(q2.w), type = tb & 3u;
        if (plane_contribution<MODE>(type, po, d0, d1, c.lights[tb >> 2], its, cam, rd, sc, recs, stack, c.w, c.n_lights_f, c.inv_gen,
                                     [&]() { const float4 q3 = pl[3]; return mkc(q3.x, q3.y, q3.z); }, cs)) n[1]++;
    }
};

template <bool LDS_SCENE, int MODE>
__global__ void __launch_bounds__(256) k_plane_gather(RenderConst rc, DeviceScene sc, StackConf stc, PlaneConst pc) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    beam_gather<LDS_SCENE>(rc, sc, stc, smem, PlaneLeaf<MODE>{pc});
}

template <bool LDS_SCENE>
static void launch_plane_impl(int mode, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PlaneConst& pc) {
    if (mode == PLANE_MODE_DISCRETE_MIS) hipLaunchKernelGGL((k_plane_gather<LDS_SCENE, PLANE_MODE_DISCRETE_MIS>), grid, block, lds_bytes, st, rc, ds, stc, pc);
    else if (mode == PLANE_MODE_CMIS) hipLaunchKernelGGL((k_plane_gather<LDS_SCENE, PLANE_MODE_CMIS>), grid, block, lds_bytes, st, rc, ds, stc, pc);
    else hipLaunchKernelGGL((k_plane_gather<LDS_SCENE, PLANE_MODE_PLAIN>), grid, block, lds_bytes, st, rc, ds, stc, pc);
}

}  // namespace rl
