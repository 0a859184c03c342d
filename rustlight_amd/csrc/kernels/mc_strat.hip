// mc_strat.hip — `ao` / `direct` with the stratified sampler (RL_STREAM_STRATIFIED, sampler.hip.h): k_pixel_mc_strat, and the sampler's test probe
// k_stratified_draws (rl_debug_stratified_draws)
#include <cstdint>

#include "common.hip.h"
#include "mc.hip.h"
#include "wavefront.h"

namespace rl {

// one lane per pixel item, samples folded in order as k_pixel_mc's per-sample form; sample s draws through StratSampler(pixel, s) on the sampler
// forked as in RL_STREAM_PER_SAMPLE
template <int KIND, bool LDS_SCENE>
__global__ void __launch_bounds__(256, LDS_SCENE ? RL_FUSED_WAVES : RL_FUSED_WAVES_STREAMING) k_pixel_mc_strat(RenderConst rc, DeviceScene sc, StackConf stc, McConst mp) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneRecs recs;
    const unsigned item = blockIdx.x * blockDim.x + threadIdx.x;
    const TravStackT<LDS_SCENE> stack = open_scene<LDS_SCENE>(sc, stc, smem, item, &recs);
    unsigned n_samples = 0, n_draws = 0, n_ext = 0, n_shadow = 0, n_vertices = 0;
    if (item < rc.n_items) {
        Rng pixel_rng = rng_seed(rc.item_seed[item], rc.seed_variant);
        const unsigned pix = rc.item_pixel[item];
        StratSampler t = strat_begin(rc, pixel_rng, item, 0u);
        Col acc = czero();
        for (unsigned s = 0; s < rc.spp; s++) {
            t.rng = rng_seed(rng_next_u64(pixel_rng), rc.seed_variant);
            t.s = s; t.used1 = 0u; t.used2 = 0u;
            acc = acc + mc_compute_pixel<KIND>(sc, recs, stack, mp, pix % rc.W, pix / rc.W, t, n_draws, n_ext, n_shadow, n_vertices);
            n_samples++;
        }
        Col px = scale_unguarded(acc, rc.inv_spp);
        rc.out[3 * (size_t)pix] = px.r; rc.out[3 * (size_t)pix + 1] = px.g; rc.out[3 * (size_t)pix + 2] = px.b;
    }
    {
        const int which[5] = {STAT_SAMPLES, STAT_VERTICES, STAT_DRAWS, STAT_SHADOW_RAYS, STAT_EXT_RAYS};
        const unsigned vals[5] = {n_samples, n_vertices, n_draws, n_shadow, n_ext};
        block_stats<5>(rc.partials, which, vals);
    }
}

void launch_pixel_mc_strat(int kind, bool lds_scene, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const McConst& mp) {
    with_flag(kind != 0, [&](auto K) { with_flag(lds_scene, [&](auto LDS) {
        hipLaunchKernelGGL((k_pixel_mc_strat<decltype(K)::value ? 1 : 0, decltype(LDS)::value>), grid, block, lds_bytes, st, rc, ds, stc, mp);
    }); });
}

// test probe: one lane per pixel walks its samples as the renderers do (pixel sampler from seeds[p], one fork per sample) and takes the call pattern
// (1 = next(), 2 = next2d()) through StratSampler; out[(p * spp + s) * n_out + j] = the j-th value sample s of pixel p drew
__global__ void __launch_bounds__(64) k_stratified_draws(RenderConst rc, unsigned n_pixels, const int* pattern, unsigned n_calls, unsigned n_out, float* out) {
    const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    Rng pixel_rng = rng_seed(rc.item_seed[p], rc.seed_variant);
    for (unsigned s = 0; s < rc.spp; s++) {
        StratSampler t = strat_begin(rc, rng_seed(rng_next_u64(pixel_rng), rc.seed_variant), p, s);
        float* o = out + ((size_t)p * rc.spp + s) * n_out;
        for (unsigned c = 0; c < n_calls; c++) {
            if (pattern[c] == 2) { const V2 v = smp_next2d(t); *o++ = v.x; *o++ = v.y; }
            else *o++ = smp_next(t);
        }
    }
}

}  // namespace rl

extern "C" int rl_debug_stratified_draws(int device, size_t n_pixels, const uint64_t* pixel_seeds, uint32_t spp, int seed_variant, size_t n_calls, const int32_t* pattern, float* out) {
    if (!pixel_seeds || !pattern || !out || n_pixels == 0 || spp == 0 || spp > (1u << 30) || n_calls == 0 || n_calls > 1024) return RL_ERR_INVALID_ARGUMENT;
    size_t n_out = 0;
    for (size_t c = 0; c < n_calls; c++) {
        if (pattern[c] != 1 && pattern[c] != 2) { rl_set_error("pattern entries are 1 (next) or 2 (next2d)"); return RL_ERR_INVALID_ARGUMENT; }
        n_out += (size_t)pattern[c];
    }
    if (n_pixels > (1u << 24) || n_pixels * spp * n_out > ((size_t)1 << 31)) { rl_set_error("probe too large"); return RL_ERR_INVALID_ARGUMENT; }
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return RL_ERR_HIP; }
    const size_t out_bytes = n_pixels * spp * n_out * sizeof(float);
    unsigned long long* d_seeds = nullptr; int* d_pat = nullptr; float* d_out = nullptr;
    int rcode = RL_OK;
    if (hipMalloc((void**)&d_seeds, n_pixels * 8) != hipSuccess || hipMalloc((void**)&d_pat, n_calls * 4) != hipSuccess || hipMalloc((void**)&d_out, out_bytes) != hipSuccess) rcode = RL_ERR_HIP;
    if (rcode == RL_OK && (hipMemcpy(d_seeds, pixel_seeds, n_pixels * 8, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_pat, pattern, n_calls * 4, hipMemcpyHostToDevice) != hipSuccess)) rcode = RL_ERR_HIP;
    if (rcode == RL_OK) {
        rl::RenderConst rc{};
        rc.spp = spp; rc.seed_variant = seed_variant; rc.item_seed = d_seeds; rc.split = 1u;
        hipLaunchKernelGGL(rl::k_stratified_draws, dim3((unsigned)((n_pixels + 63) / 64)), dim3(64), 0, 0, rc, (unsigned)n_pixels, d_pat, (unsigned)n_calls, (unsigned)n_out, d_out);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost) != hipSuccess) rcode = RL_ERR_HIP;
    }
    if (rcode != RL_OK) { (void)hipGetLastError(); rl_set_error("rl_debug_stratified_draws: HIP error"); }
    if (d_seeds) hipFree(d_seeds);
    if (d_pat) hipFree(d_pat);
    if (d_out) hipFree(d_out);
    return rcode;
}
