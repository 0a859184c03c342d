// fused.hip.h — k_path_fused, the persistent form of the pipeline, and its launcher; instantiated by fused_lds.hip (scene staged in LDS)
// and fused_stream.hip (BVH streamed from L2 / HBM) so that the two families compile in parallel, and once more each by fused_*_fast.hip with
// RL_FAST_MATH (NUM = 1: the opt-in tolerance build; the template parameter only keeps the kernel symbols of the two builds apart).
#pragma once
#ifdef RL_STAGE_TIMERS
#include <algorithm>
#include <cstdlib>
#include <vector>
#endif

#ifndef RL_FUSED_QUEUE
#define RL_FUSED_QUEUE 0    // 1 (fusedq_lds.hip / fusedq_stream.hip): this translation unit instantiates the queue-fed form of the kernel
#endif

namespace rl {

// ------------------------------------------------------------------------------------------
// k_path_fused<MAT, MEDIUM, LDS> — the persistent form of the pipeline for scenes with one BSDF type: one
// launch, one lane per pixel item, the four stage functions above run back-to-back per iteration
// (raygen -> extend -> shade -> shadow) with the path state in registers and LDS (FusedState) and the scene +
// traversal stacks in LDS.  Same functions, same order of operations, same results as the wavefront kernels;
// what disappears is ~1.4 KB/sample of state traffic through HBM and ~2000 kernel boundaries per render.
#ifdef RL_STAGE_TIMERS
__device__ unsigned long long g_stage_timers[32];      // [0..3] cycles per stage, [4..7] live lanes per stage, [8] lane slots, [9..15] the shadow stage's loops, [16..] shadow-stage occupancy (dump_stage_timers_impl)
static constexpr unsigned kFusedWgSlots = 1u << 15;
static __device__ unsigned long long g_fused_wgs[2 * kFusedWgSlots];      // per workgroup (start, end) on the 100 MHz wall clock: the launch's drain (dump_stage_timers_impl; as g_chain_waves of chain.hip.h)
#endif
// QUEUE: the form that takes its work from the chain pass's completion queue (the evaluation pass of reference-order streams, launched beside the chain pass): an
// instantiation of its own (fusedq_lds.hip / fusedq_stream.hip), so that the per-sample kernel's code is exactly what it is without it.
// NUM + 2 (LDS-staged scenes without a medium only; NUM is a symbol tag, 0 = exact and 1 = tolerance build, and bit 1 of it is this form's — a bool parameter of its
// own would rename every instantiation the resource table and its test know by name): the form whose last heavy tiles run at several lanes per pixel (raygen_slot<.., TAIL>; RenderConst::tail_*), an
// instantiation of its own for the same reason — launched when the render has a tail, so that a render without one runs the kernel it always ran.
// The body is fused_body.inc.h: k_path_fused includes it with the independent sampler (SMP = Rng), k_path_fused_strat (fused_strat.hip.h) with StratSampler.
template <int MAT, bool MEDIUM, bool LDS_SCENE, int LIGHTS, int NUM, bool QUEUE = false>
__global__ void __launch_bounds__(256, LDS_SCENE ? RL_FUSED_WAVES : RL_FUSED_WAVES_STREAMING) k_path_fused(RenderConst rc_arg, DeviceScene sc_arg, StackConf stc) {
    using SMP = Rng;
#define RL_FUSED_BODY_TAIL ((NUM & 2) != 0 && !QUEUE && LDS_SCENE && !MEDIUM)
#include "fused_body.inc.h"
#undef RL_FUSED_BODY_TAIL
}


template <bool LDS_SCENE>
static void launch_fused_impl(int mat, bool medium, bool area_only, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc) {
    with_bsdf(mat, [&](auto M) { with_flag(medium, [&](auto MED) { with_flag(area_only, [&](auto AREA) { with_flag(rc.tail_lanes != 0u, [&](auto TAIL) {
        constexpr int MAT = decltype(M)::value, LIGHTS = decltype(AREA)::value ? LIGHTS_AREA_ONLY : LIGHTS_ANY;
        constexpr int NUM = RL_NUMERICS_ID + ((decltype(TAIL)::value && LDS_SCENE && !decltype(MED)::value && RL_FUSED_QUEUE == 0) ? 2 : 0);      // (the host plans a tail for these forms only)
        hipLaunchKernelGGL((k_path_fused<MAT, decltype(MED)::value, LDS_SCENE, LIGHTS, NUM, RL_FUSED_QUEUE != 0>), grid, block, lds_bytes, st, rc, ds, stc);
    }); }); }); });
}
template <bool LDS_SCENE>
static void dump_stage_timers_impl() {
#ifdef RL_STAGE_TIMERS
    // dev-only build: per-stage cycle shares and active-lane fractions of the fused loop
    unsigned long long h[32];
    hipMemcpyFromSymbol(h, HIP_SYMBOL(g_stage_timers), sizeof(h));
    const double tot = (double)(h[0] + h[1] + h[2] + h[3]);
    const char* names[4] = {"raygen", "extend", "shade", "shadow"};
    for (int k = 0; k < 4; k++) std::fprintf(stderr, "[stage] %-7s cycles %5.1f %%  lanes %5.1f %%\n", names[k], 100.0 * h[k] / tot, 100.0 * h[4 + k] / (double)h[8]);
    {
        const double it = (double)(h[16] + h[17] + h[18] + h[19] + h[20]), ex = it - (double)h[16], pr = (double)(h[21] + h[22] + h[23] + h[24]);
        if (it > 0) std::fprintf(stderr, "[stage] shadow stage: runs in %.1f %% of the wave-iterations; where it runs the wave holds 1-16 / 17-32 / 33-48 / 49-64 shadow rays in %.1f / %.1f / %.1f / %.1f %% (%.1f lanes on average)\n",
                                 100.0 * ex / it, 100.0 * h[17] / std::max(1.0, ex), 100.0 * h[18] / std::max(1.0, ex), 100.0 * h[19] / std::max(1.0, ex), 100.0 * h[20] / std::max(1.0, ex), (double)h[7] / std::max(1.0, ex));
        if (ex > 0) std::fprintf(stderr, "[stage] shadow loops, means per execution of the stage: node trips the wave paid %.2f, triangle-test iterations it paid %.2f, largest per-lane node trips %.2f, "
                                 "candidate triangles of all lanes %.2f (largest per lane %.2f), packed rounds %.2f in %.2f passes\n",
                                 (double)h[9] / ex, (double)h[10] / ex, (double)h[11] / ex, (double)h[12] / ex, (double)h[13] / ex, (double)h[14] / ex, (double)h[15] / ex);
        if (pr > 0) std::fprintf(stderr, "[stage] pairs of consecutive iterations: neither holds shadow rays %.1f %%, one does %.1f %%, both and <= 64 together %.1f %% (one traversal could serve both), both and > 64 %.1f %%\n",
                                 100.0 * h[21] / pr, 100.0 * h[22] / pr, 100.0 * h[23] / pr, 100.0 * h[24] / pr);
    }
    std::memset(h, 0, sizeof(h)); hipMemcpyToSymbol(HIP_SYMBOL(g_stage_timers), h, sizeof(h));
    {   // the end of the launch: lifetimes of the heavy workgroups (those that live at least a quarter of the p90 lifetime), the busy workgroup slots over the last
        // 1.5 median lifetimes and the idle slot-time there (profiles/fused_tail_note.md)
        std::vector<unsigned long long> w(2 * (size_t)kFusedWgSlots);
        hipMemcpyFromSymbol(w.data(), HIP_SYMBOL(g_fused_wgs), w.size() * 8);
        std::vector<std::pair<double, double>> wg;      // (start, end) in ms from the first start
        unsigned long long t_first = ~0ull;
        for (size_t i = 0; i < kFusedWgSlots; i++) if (w[2 * i + 1]) t_first = std::min(t_first, w[2 * i]);
        for (size_t i = 0; i < kFusedWgSlots; i++) if (w[2 * i + 1]) wg.push_back({(w[2 * i] - t_first) * 1e-5, (w[2 * i + 1] - t_first) * 1e-5});
        int dev = 0, cus = 256;
        (void)hipGetDevice(&dev); (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        const double slots = (double)cus * (LDS_SCENE ? RL_FUSED_WAVES : RL_FUSED_WAVES_STREAMING);
        if (wg.size() >= 16) {
            auto pct = [](std::vector<double> v, double q) { std::sort(v.begin(), v.end()); return v[std::min(v.size() - 1, (size_t)(q * (double)v.size()))]; };
            std::vector<double> life, heavy;
            double span = 0.0, busy_total = 0.0, last_heavy_start = 0.0;
            for (const auto& g : wg) { life.push_back(g.second - g.first); span = std::max(span, g.second); busy_total += g.second - g.first; }
            const double cut = 0.25 * pct(life, 0.9);
            for (const auto& g : wg) if (g.second - g.first >= cut) { heavy.push_back(g.second - g.first); last_heavy_start = std::max(last_heavy_start, g.first); }
            const double L = pct(heavy, 0.5), L90 = pct(heavy, 0.9), win0 = std::max(0.0, span - 1.5 * L);
            double busy_win = 0.0;
            for (const auto& g : wg) busy_win += std::max(0.0, g.second - std::max(g.first, win0));
            std::fprintf(stderr, "[tail] %zu workgroups (%zu heavy) on %.0f slots, launch %.3f ms; heavy lifetime median %.3f ms, p90 %.3f ms, max %.3f ms; last heavy workgroup starts at %.3f ms\n",
                         wg.size(), heavy.size(), slots, span, L, L90, pct(heavy, 1.0), last_heavy_start);
            std::fprintf(stderr, "[tail] busy slots over the last 1.5 L (from %.3f ms, every L / 8):", win0);
            for (int k = 0; k <= 12; k++) { const double t = win0 + (span - win0) * k / 12.0; unsigned n = 0; for (const auto& g : wg) if (g.first <= t && t < g.second) n++; std::fprintf(stderr, " %u", n); }
            std::fprintf(stderr, "\n[tail] idle slot-time in that window %.2f slot-ms = %.2f %% of slots x launch; over the whole launch %.2f %%\n",
                         slots * (span - win0) - busy_win, 100.0 * (slots * (span - win0) - busy_win) / (slots * span), 100.0 * (slots * span - busy_total) / (slots * span));
        }
        std::fill(w.begin(), w.end(), 0ull); hipMemcpyToSymbol(HIP_SYMBOL(g_fused_wgs), w.data(), w.size() * 8);
    }
#endif
}

}  // namespace rl
