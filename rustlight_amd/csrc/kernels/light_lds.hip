// light_lds.hip — k_light_fused for scenes staged in LDS, and k_light_resolve; see light.hip.h
#include "common.hip.h"
#include "light.hip.h"

namespace rl {

// k_light_resolve — the 96-bit fixed-point sums to the f32 image, times 1 / spp (light.rs:292-296: Σ splats · W·H / paths traced); a flagged channel
// is +inf.  carry * 2^64 is exact in f64, so the sum's only roundings are (double)low and the add.
__global__ void __launch_bounds__(256) k_light_resolve(RenderConst rc, LightConst lc) {
    const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= (size_t)rc.W * rc.H) return;
    const unsigned flags = lc.inf_flags[pix];
    for (int k = 0; k < 3; k++) {
        const double sum = (double)lc.carry[3 * pix + k] * 18446744073709551616.0 + (double)lc.accum[3 * pix + k];
        const double v = sum * (1.0 / (double)(1ll << kLightFixBits)) / (double)rc.spp;
        rc.out[3 * pix + k] = (flags >> k) & 1u ? f32_inf() : (float)v;
    }
}

void launch_light_lds(int mat, bool medium, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const LightConst& lc) {
    launch_light_impl<true>(mat, medium, grid, block, lds_bytes, st, rc, ds, stc, lc);
}
void launch_light_resolve(dim3 grid, dim3 block, hipStream_t st, const RenderConst& rc, const LightConst& lc) {
    hipLaunchKernelGGL(k_light_resolve, grid, block, 0, st, rc, lc);
}

}  // namespace rl
