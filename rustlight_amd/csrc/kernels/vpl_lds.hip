// vpl_lds.hip — the VPL kernels for scenes staged in LDS, and k_vpl_resolve; see vpl.hip.h
#include "common.hip.h"
#include "vpl.hip.h"

namespace rl {

// k_vpl_resolve — workgroup = owned block, lane c = ix * bh + iy as in k_vpl_primary: im_block.scale(1 / spp) into the image
__global__ void __launch_bounds__(256) k_vpl_resolve(RenderConst rc, VplConst vc) {
    const unsigned ob = blockIdx.x, c = threadIdx.x;
    unsigned bx, by, bw, bh;
    block_geometry(rc, rc.owned_blocks[ob], &bx, &by, &bw, &bh);
    if (c >= bw * bh) return;
    const unsigned item = rc.block_item_base[ob] + c;
    const Col a = mkc(vc.acc[3 * (size_t)item], vc.acc[3 * (size_t)item + 1], vc.acc[3 * (size_t)item + 2]);
    const Col px = scale_unguarded(a, rc.inv_spp);
    const size_t pix = (size_t)(by + c % bh) * rc.W + (bx + c / bh);
    rc.out[3 * pix] = px.r; rc.out[3 * pix + 1] = px.g; rc.out[3 * pix + 2] = px.b;
}

void launch_vpl_lds(int which, int mat, bool medium, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const VplConst& vc) {
    launch_vpl_impl<true>(which, mat, medium, grid, block, lds_bytes, st, rc, ds, stc, vc);
}
void launch_vpl_resolve(dim3 grid, dim3 block, hipStream_t st, const RenderConst& rc, const VplConst& vc) {
    hipLaunchKernelGGL(k_vpl_resolve, grid, block, 0, st, rc, vc);
}
}  // namespace rl
