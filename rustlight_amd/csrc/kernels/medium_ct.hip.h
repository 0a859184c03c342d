// medium_ct.hip.h — medium_sample (shading.hip.h) with the one field it drops: continued_t, the distance HomogenousVolume::sample draws before it is cut at the
// ray's max_t (src/volume.rs:102-130).  A sibling, not an edit: the kernels that inline medium_sample stay as they are.  Statement for statement medium_sample,
// so t, w and exited are its bits.
#pragma once

namespace rl {

struct MediumSampleCt { float t; Col w; bool exited; float continued_t; };
RL_DEV MediumSampleCt medium_sample_ct(const MediumRecord& m, float max_t, float u) {
    Col sigma_t = mkc(m.sigma_t[0], m.sigma_t[1], m.sigma_t[2]);
    Col sigma_s = mkc(m.sigma_s[0], m.sigma_s[1], m.sigma_s[2]);
    float u3 = u * 3.0f;
    int component = u3 != u3 ? 0 : (u3 <= 0.0f ? 0 : (u3 >= 255.0f ? 255 : (int)u3));   // `as u8`
    u = u * 3.0f - (float)component;
    float sigma_t_c = cget(sigma_t, component);
    float t = div_rn(-m_logf(1.0f - u), sigma_t_c);
    float t_min = rmin(t, max_t);
    bool exited = t >= max_t;
    Col tau = t_min * sigma_t;
    Col w = cexp(-tau);
    float pdf;
    if (exited) pdf = cavg(cexp(-tau));
    else { w = w * sigma_s; pdf = cavg(sigma_t * cexp(-tau)); }
    w = div_unguarded(w, pdf);
    MediumSampleCt r; r.t = t_min; r.w = w; r.exited = exited; r.continued_t = t;
    return r;
}

}  // namespace rl
