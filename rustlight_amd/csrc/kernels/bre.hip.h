// bre.hip.h — the beam radiance estimate of IntegratorVolPrimitives (src/integrators/explicit/vol_primitives.rs:41-98, 712-790): the volume photons of a
// light pass (the records of rl_vpl_generate with RL_VPL_VOLUME: convert_photons stores what convert_vpl stores under `-v volume`) are gathered along every
// camera ray through a tree of photon spheres (host/photontree.cpp).  The gather is beam_gather (gather.hip.h) over the leaf below.  Instantiated by
// bre_lds.hip (scene staged in LDS) and bre_stream.hip (BVH streamed from L2 / HBM).
//
// Photon: 3 float4 = pos | radiance | d_in; the radiance is loaded for accepted photons only, d_in only by the Henyey-Greenstein instantiation.
#pragma once
#include "gather.hip.h"

namespace rl {

// HG: the medium's phase function is Henyey-Greenstein
template <bool HG>
struct BreLeaf {
    BreConst c;
    static constexpr int kCounters = 1;                                     // photons gathered
    static constexpr int kLo[1] = {STAT_BRE_PHOTONS}, kHi[1] = {STAT_BRE_PHOTONS_HI};
    template <class STACK>
    RL_DEV void element(unsigned idx, V3 cam, V3 rd, float tfar, const DeviceScene& sc, const SceneRecs&, const STACK&, Col& cs, unsigned long long (&n)[1]) const {
        const float4* ph = c.photons + 3u * (size_t)idx;
        const float4 q0 = ph[0];
        const V3 pos = mk3(q0.x, q0.y, q0.z);
        const float along = dot(pos - cam, rd);                            // Photon::intersection (vol_primitives.rs:63-78)
        if (along <= 0.0f || along > tfar) return;
        const V3 p = cam + rd * along;
        if (length2(pos - p) > c.radius2) return;
        n[0]++;
        const float4 q1 = ph[1];                                            // Photon::contribute (81-98), then `* norm_photon`
        const Col trans = medium_transmittance(sc.medium, along);
        Col phase;
        if (HG) { const float4 q2 = ph[2]; phase = phase_eval(sc.medium, -rd, mk3(q2.x, q2.y, q2.z)); }
        else phase = cval(div_rn(1.0f, kPi * 4.0f));
        cs = cs + (((mkc(q1.x, q1.y, q1.z) * trans) * phase) * c.kernel) * c.norm_photon;
    }
};

template <bool LDS_SCENE, bool HG>
__global__ void __launch_bounds__(256) k_bre_gather(RenderConst rc, DeviceScene sc, StackConf stc, BreConst bc) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    beam_gather<LDS_SCENE>(rc, sc, stc, smem, BreLeaf<HG>{bc});
}

template <bool LDS_SCENE>
static void launch_bre_impl(bool hg, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const BreConst& bc) {
    with_flag(hg, [&](auto H) { hipLaunchKernelGGL((k_bre_gather<LDS_SCENE, decltype(H)::value>), grid, block, lds_bytes, st, rc, ds, stc, bc); });
}

}  // namespace rl
