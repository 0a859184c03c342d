// beam.hip.h — the photon beams' gather (src/integrators/explicit/vol_primitives.rs:101-199, 705-790, `Beams` arm): the sub-beams of a beam pass, split and
// sorted into BHVAccel's tree on the host (host/beamtree.cpp), are gathered along every camera ray.  The gather is beam_gather (gather.hip.h) over the leaf
// below.  Instantiated by beam_lds.hip (scene staged in LDS) and beam_stream.hip (BVH streamed from L2 / HBM).
//
// Sub-beam: 3 float4 = o, length | d, 0 | radiance, 0; the radiance is loaded for accepted beams only.  A beam's phase function is Isotropic whatever the
// medium's is (convert_beams stores PhaseFunction::Isotropic(), vol_primitives.rs:457, 483, 500): no Henyey-Greenstein instantiation.
#pragma once
#include "gather.hip.h"

namespace rl {

struct BeamLeaf {
    BeamConst c;
    static constexpr int kCounters = 1;                                     // beams accepted
    static constexpr int kLo[1] = {STAT_BEAM_ACCEPTED}, kHi[1] = {STAT_BEAM_ACCEPTED_HI};
    template <class STACK>
    RL_DEV void element(unsigned idx, V3 cam, V3 rd, float tfar, const DeviceScene& sc, const SceneRecs&, const STACK&, Col& cs, unsigned long long (&n)[1]) const {
        const float4* bm = c.beams + 3u * (size_t)idx;
        const float4 q0 = bm[0], q1 = bm[1];
        const V3 bo = mk3(q0.x, q0.y, q0.z), bd = mk3(q1.x, q1.y, q1.z);
        const float len = q0.w;
        // PhotonBeam::intersection (vol_primitives.rs:140-181)
        const V3 d1d2c = cross(rd, bd);
        const float sin_theta_sqr = length2(d1d2c);
        const float ad = dot(bo - cam, d1d2c);
        if (ad * ad >= c.radius2 * sin_theta_sqr) return;                  // lines too far apart
        const float d1d2 = dot(rd, bd);
        const float d1d2_sqr = d1d2 * d1d2;
        const float d1d2_sqr_minus1 = d1d2_sqr - 1.0f;
        if (d1d2_sqr_minus1 < 1e-5f && d1d2_sqr_minus1 > -1e-5f) return;   // parallel lines
        const float d1o1 = dot(rd, cam);
        const float d1o2 = dot(rd, bo);
        const float w = div_rn(d1o1 - d1o2 - d1d2 * (dot(bd, cam) - dot(bd, bo)), d1d2_sqr_minus1);
        if (w <= kEps || w >= tfar) return;                                // r.tnear (Ray::new: constants::EPSILON), r.tfar
        const float v = div_rn(w + d1o1 - d1o2, d1d2);
        if (v <= 0.0f || v >= len || !finite_f(v)) return;
        const float sin_theta = sqrt_rn(sin_theta_sqr);
        n[0]++;
        // PhotonBeam::contribute (184-199), then `* norm_photon`
        const float4 q2 = bm[2];
        const Col trans = medium_transmittance(sc.medium, w);
        const Col phase_func = mkc(sc.medium.sigma_s[0], sc.medium.sigma_s[1], sc.medium.sigma_s[2]) * cval(div_rn(1.0f, kPi * 4.0f));
        const float weight = div_rn(1.0f, sin_theta) * c.half_inv_radius;
        cs = cs + (((mkc(q2.x, q2.y, q2.z) * trans) * phase_func) * weight) * c.norm_photon;
    }
};

template <bool LDS_SCENE>
__global__ void __launch_bounds__(256) k_beam_gather(RenderConst rc, DeviceScene sc, StackConf stc, BeamConst bc) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    beam_gather<LDS_SCENE>(rc, sc, stc, smem, BeamLeaf{bc});
}

}  // namespace rl
