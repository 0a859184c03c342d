// shade.hip — the shading kernels of the wavefront pipeline: k_shade<MAT, MEDIUM> (single-BSDF scenes) and k_shade_sorted (material sort)
#include "common.hip.h"
#include "shade_sorted.hip.h"

namespace rl {

// k_shade<MAT, MEDIUM>: scenes with a single BSDF type — every live slot goes straight to that BSDF's code.
template <int MAT, bool MEDIUM>
__global__ void __launch_bounds__(256) k_shade(RenderConst rc, DeviceScene sc, Pool pool) {
    unsigned slot = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned n_vertices = 0, n_draws = 0, n_shadow = 0, n_ext = 0;
    PoolState ps{pool, slot};
    unsigned flags = slot < pool.P ? PU(U_FLAGS) : 0u;
    if (flags & ST_RAY) shade_slot<MAT, MEDIUM>(rc, sc, ps, flags, n_vertices, n_draws, n_shadow, n_ext);
    {
        const int which[4] = {STAT_VERTICES, STAT_DRAWS, STAT_SHADOW_RAYS, STAT_EXT_RAYS};
        const unsigned vals[4] = {n_vertices, n_draws, n_shadow, n_ext};
        block_stats<4>(rc.partials, which, vals);
    }
}

// k_shade_sorted<MEDIUM, CHUNKS>: mixed-material scenes (shade_sorted.hip.h)
template <bool MEDIUM, unsigned CHUNKS>
__global__ void __launch_bounds__(256, RL_SORT_WAVES) k_shade_sorted(RenderConst rc, DeviceScene sc, Pool pool) {
    using SMP = Rng;
#include "shade_sorted_body.inc.h"
}

template <int MAT>
static void launch_shade(bool medium, dim3 grid, dim3 block, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const Pool& pool) {
    if (medium) hipLaunchKernelGGL((k_shade<MAT, true>), grid, block, 0, st, rc, ds, pool);
    else hipLaunchKernelGGL((k_shade<MAT, false>), grid, block, 0, st, rc, ds, pool);
}
void launch_shade_type(int type, bool medium, dim3 grid, dim3 block, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const Pool& pool) {
    switch (type) {
        case BSDF_DIFFUSE: launch_shade<BSDF_DIFFUSE>(medium, grid, block, st, rc, ds, pool); break;
        case BSDF_PHONG: launch_shade<BSDF_PHONG>(medium, grid, block, st, rc, ds, pool); break;
        case BSDF_METAL: launch_shade<BSDF_METAL>(medium, grid, block, st, rc, ds, pool); break;
        case BSDF_GLASS: launch_shade<BSDF_GLASS>(medium, grid, block, st, rc, ds, pool); break;
        default: launch_shade<BSDF_SUBSTRATE>(medium, grid, block, st, rc, ds, pool); break;
    }
}


void launch_shade_sorted(bool medium, unsigned chunks, dim3 grid, dim3 block, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const Pool& pool) {
    if (chunks == 4u) {
        if (medium) hipLaunchKernelGGL((k_shade_sorted<true, 4>), grid, block, 0, st, rc, ds, pool);
        else hipLaunchKernelGGL((k_shade_sorted<false, 4>), grid, block, 0, st, rc, ds, pool);
    } else {
        if (medium) hipLaunchKernelGGL((k_shade_sorted<true, 1>), grid, block, 0, st, rc, ds, pool);
        else hipLaunchKernelGGL((k_shade_sorted<false, 1>), grid, block, 0, st, rc, ds, pool);
    }
}

}  // namespace rl
