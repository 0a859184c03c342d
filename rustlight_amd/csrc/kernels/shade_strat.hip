// shade_strat.hip — the wavefront pipeline's sampler-dependent kernels with the stratified sampler (RL_STREAM_STRATIFIED, sampler.hip.h):
// k_raygen_strat (k_raygen's loop) and k_shade_sorted_strat (shade_sorted.hip.h; every scene, a single BSDF type included — a specialised MAT never
// changes an image).  k_init, k_extend, k_shadow and k_fold_samples draw nothing and are shared with the independent sampler.
#include "common.hip.h"
#include "shade_sorted.hip.h"

namespace rl {

__global__ void __launch_bounds__(256) k_raygen_strat(RenderConst rc, DeviceScene sc, Pool pool) {
    unsigned n_samples = 0, n_draws = 0;
    for (unsigned slot = blockIdx.x * blockDim.x + threadIdx.x; slot < pool.P; slot += gridDim.x * blockDim.x) {
        PoolState ps{pool, slot};
        raygen_slot<true, PoolState, StratSampler>(rc, sc, ps, n_samples, n_draws);
    }
    { const int which[2] = {STAT_SAMPLES, STAT_DRAWS}; const unsigned vals[2] = {n_samples, n_draws}; block_stats<2>(rc.partials, which, vals); }
}

template <bool MEDIUM, unsigned CHUNKS>
__global__ void __launch_bounds__(256, RL_SORT_WAVES) k_shade_sorted_strat(RenderConst rc, DeviceScene sc, Pool pool) {
    using SMP = StratSampler;
#include "shade_sorted_body.inc.h"
}

void launch_raygen_strat(dim3 grid, dim3 block, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const Pool& pool) {
    hipLaunchKernelGGL(k_raygen_strat, grid, block, 0, st, rc, ds, pool);
}
void launch_shade_sorted_strat(bool medium, unsigned chunks, dim3 grid, dim3 block, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const Pool& pool) {
    if (chunks == 4u) {
        if (medium) hipLaunchKernelGGL((k_shade_sorted_strat<true, 4>), grid, block, 0, st, rc, ds, pool);
        else hipLaunchKernelGGL((k_shade_sorted_strat<false, 4>), grid, block, 0, st, rc, ds, pool);
    } else {
        if (medium) hipLaunchKernelGGL((k_shade_sorted_strat<true, 1>), grid, block, 0, st, rc, ds, pool);
        else hipLaunchKernelGGL((k_shade_sorted_strat<false, 1>), grid, block, 0, st, rc, ds, pool);
    }
}

}  // namespace rl
