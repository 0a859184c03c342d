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

// (no k_shade<-1>: a scene that mixes BSDF types, or a type this build does not know, is shaded by the material sort, one slot per lane)
void launch_shade_type(int type, bool medium, dim3 grid, dim3 block, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const Pool& pool) {
    with_bsdf(type, [&](auto M) {
        if constexpr (decltype(M)::value < 0) launch_shade_sorted(medium, 1u, grid, block, st, rc, ds, pool);
        else with_flag(medium, [&](auto MED) { hipLaunchKernelGGL((k_shade<decltype(M)::value, decltype(MED)::value>), grid, block, 0, st, rc, ds, pool); });
    });
}

void launch_shade_sorted(bool medium, unsigned chunks, dim3 grid, dim3 block, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const Pool& pool) {
    with_flag(chunks == 4u, [&](auto FOUR) { with_flag(medium, [&](auto MED) {
        hipLaunchKernelGGL((k_shade_sorted<decltype(MED)::value, decltype(FOUR)::value ? 4u : 1u>), grid, block, 0, st, rc, ds, pool);
    }); });
}

}  // namespace rl
