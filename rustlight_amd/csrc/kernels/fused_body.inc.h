// fused_body.inc.h — the body of k_path_fused / k_path_fused_strat (fused.hip.h, fused_strat.hip.h), included inside the kernel: the kernel defines `SMP`
// (the sampler, sampler.hip.h) and the template parameters MAT, MEDIUM, LDS_SCENE, LIGHTS, QUEUE, and takes (RenderConst rc_arg, DeviceScene sc_arg, StackConf stc).
// (Text included, not a function called: an inlined device function with the same statements allocates the kernel's registers differently.)
    const RenderConst& rc = rc_arg;
    const DeviceScene& sc = sc_arg;
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    // (open_scene of stages.hip.h, written out: called as a function it gives this kernel other instructions, and the published numbers are this kernel's)
    SceneRecs recs;
    float4* after_scene = smem;
    if (LDS_SCENE) {
        stage_scene_lds(sc, smem, smem + lds_nodes_float4s(sc.n_nodes));
        recs.nodes = smem; recs.tris = smem + lds_nodes_float4s(sc.n_nodes);
        after_scene = smem + lds_scene_float4s(sc.n_nodes, sc.n_prims);
    } else {
        recs.nodes = streamed_nodes<TravStackT<false>>(sc);   // exact build: BVH2 nodes; tolerance build: quantised BVH4 nodes
        recs.tris = reinterpret_cast<const float4*>(sc.tris);
    }
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x;
    // LDS: [scene][cold path state (u64 | f32 | u32 planes)][per-lane stacks]
    unsigned long long* cold_q = reinterpret_cast<unsigned long long*>(after_scene);
    float* cold_f = reinterpret_cast<float*>(cold_q + 256 * FusedState::kColdQ);
    unsigned* cold_u = reinterpret_cast<unsigned*>(cold_f + 256 * FusedState::kColdF);
    const TravStackT<LDS_SCENE> stack(make_stack<LDS_SCENE>(stc, cold_u + 256 * FusedState::kColdU, tid));
    FusedState ps;
    ps.cold_q = cold_q + threadIdx.x; ps.cold_f = cold_f + threadIdx.x; ps.cold_u = cold_u + threadIdx.x;
#pragma unroll
    for (int i = 0; i < F_COUNT; i++) ps.fv[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < U_COUNT; i++) ps.uv[i] = 0u;
#pragma unroll
    for (int i = 0; i < Q_COUNT; i++) ps.qv[i] = 0ull;
    storec(ps, F_AR, czero());
    PU(U_CURSOR) = 0u; PU(U_SAMPLE) = 0u;
    // few work items (reference-order streams: one per 16x16 block, 8160 at 1080p): they are dealt to every 2^item_shift-th lane, so that
    // they spread over as many waves as the chip holds — a wave's speed does not depend on how many of its lanes are live, and a SIMD
    // needs 2-3 ready waves to issue at its rate (profiles/r02_valu_calibration.json)
    const unsigned item0 = (tid & ((1u << rc.item_shift) - 1u)) == 0u ? (tid >> rc.item_shift) : 0xffffffffu;
    PU(U_ITEM) = item0;
    PU(U_PRIM) = 0xffffffffu;
    PU(U_FLAGS) = item0 < rc.n_items ? (ST_REGEN | ST_FRESH) : ST_FINISHED;
    unsigned n_samples = 0, n_draws = 0, n_vertices = 0, n_shadow = 0, n_ext = 0;
#ifdef RL_STAGE_TIMERS
    unsigned long long tm[4] = {0, 0, 0, 0}, ln[5] = {0, 0, 0, 0, 0};
    // the shadow stage where it runs: wave-iterations by the number of lanes that hold a shadow ray (0 | 1-16 | 17-32 | 33-48 | 49-64), and what packing the shadow rays of
    // TWO consecutive iterations into one traversal could save: pairs of iterations by (both empty | one empty | both hold rays and together <= 64 | together > 64)
    unsigned long long sh_hist[5] = {0, 0, 0, 0, 0}, sh_pair[4] = {0, 0, 0, 0}, sh_cyc_exec = 0; unsigned sh_prev = 0, sh_parity = 0;
    // ... and its loops, summed over the executions (PackStats): [0] node trips the wave paid, [1] triangle-test iterations it paid, [2] the largest per-lane count of inner-node
    // trips, [3] candidate triangles of all lanes (packed form: of the full enumeration; per-lane loop: triangles tested), [4] the largest per-lane count, [5] packed rounds, [6] passes of phase B
    unsigned long long sh_loop[7] = {0, 0, 0, 0, 0, 0, 0};
#define RL_T0 { t0 = __builtin_readcyclecounter(); }
#define RL_T1(K, COND) { unsigned long long t1 = __builtin_readcyclecounter(); tm[K] += t1 - t0; ln[K] += __popcll(__ballot(COND)); t0 = t1; }
    unsigned long long t0;
    const unsigned long long wg_t0 = wall_clock64();
#else
#define RL_T0
#define RL_T1(K, COND)
#endif
    // ---- QUEUE form (the evaluation pass of reference-order streams beside the chain pass): the lanes take their pixel items from this launch's block list — item
    // position c = block c / (256 split) of the list, item c % (256 split) of that block — through one claim counter, like the dispenser's lanes; every block of the list is
    // complete (the host only lists blocks the chain kernel has flagged), so nothing here waits.
    constexpr bool qmode = QUEUE;
    constexpr unsigned kQDone = 0xffffffffu;
    if constexpr (qmode) {
        PU(U_ITEM) = 0u;
        PU(U_FLAGS) = ST_FINISHED;           // "needs a claim"
    }
    for (;;) {
    if constexpr (qmode) {
        // (the render constants re-read from the kernarg segment, like the loop body does: kept in scalar registers across the loop they cost the medium kernel 82 spilled SGPRs)
        const char __attribute__((address_space(4)))* kq = (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kq));
        const RenderConst& rc_arg = *(const RenderConst*)kq;
        const unsigned ipb = 256u * rc_arg.split, total = rc_arg.q_n * ipb;
        unsigned fl = PU(U_FLAGS);
        for (int tries = 0; tries < 4; tries++) {       // (a claim can land past the end of a ragged block: claim again, a few times per trip)
            if ((fl & ST_FINISHED) && PU(U_ITEM) != kQDone) {
                const unsigned c = atomicAdd(rc_arg.q_ctr, 1u);
                if (c >= total) PU(U_ITEM) = kQDone;
                else {
                    const unsigned j = rc_arg.q_list[c / ipb], idx = c - (c / ipb) * ipb;
                    unsigned bx_, by_, bw_, bh_;
                    block_geometry(rc_arg, rc_arg.owned_blocks[j], &bx_, &by_, &bw_, &bh_);
                    const unsigned npx = min(rc_arg.cursor_end, bw_ * bh_) - min(rc_arg.cursor_begin, bw_ * bh_);
                    if (idx < npx * rc_arg.split) {
                        PU(U_ITEM) = rc_arg.block_item_base[j] * rc_arg.split + idx;
                        PU(U_PRIM) = 0xffffffffu; PU(U_CURSOR) = 0u; PU(U_SAMPLE) = 0u;
                        storec(ps, F_AR, czero());
                        fl = ST_REGEN | ST_FRESH;
                    }                                   // else: past the block's last pixel, claim again
                }
            }
            if (__ballot((fl & ST_FINISHED) && PU(U_ITEM) != kQDone) == 0ull) break;
        }
        PU(U_FLAGS) = fl;
        if (__ballot(!(fl & ST_FINISHED)) == 0ull) {
            if (__ballot((fl & ST_FINISHED) && PU(U_ITEM) != kQDone) == 0ull) break;      // every lane of the wave is done
            continue;                                                                      // (only claims past ragged ends so far: claim on)
        }
    }
    // (queue mode: ONE trip of the loop body, then back to the claims — a lane whose pixel is done takes its next item while the others go on, like the dispenser's lanes)
    if (!(PU(U_FLAGS) & ST_FINISHED)) do {
        // The scene record (25 pointers, camera matrices, ...) and the render constants do not fit the scalar registers next to the saved
        // exec masks of the stage functions: kept live across the loop they are spilled to VGPR lanes (v_writelane / v_readlane were ~600 of
        // the kernel's ~4500 vector instructions, 126 spilled SGPRs).  Re-deriving their address from the kernarg segment once per iteration
        // lets the compiler s_load what each stage needs instead (0-22 spilled SGPRs, 2-6 spilled VGPRs instead of 21; cbox 55.8 -> 51.9 ms,
        // cbox + medium 136.0 -> 118.9 ms at 32 spp, same bits).  The render constants are re-read too where that paid (the medium kernels).
        const char __attribute__((address_space(4)))* ka = (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka));
        constexpr size_t sc_off = (sizeof(RenderConst) + alignof(DeviceScene) - 1) / alignof(DeviceScene) * alignof(DeviceScene);
        static_assert(sc_off == offsetof(PathKernargs, sc) && offsetof(PathKernargs, rc) == 0, "kernarg layout of k_path_fused(RenderConst, DeviceScene, StackConf)");
        const DeviceScene& sc = *(const DeviceScene*)(ka + sc_off);
        const RenderConst& rc = MEDIUM ? *(const RenderConst*)ka : rc_arg;
        RL_T0
#ifdef RL_STAGE_TIMERS
        ln[4] += 64;
        const bool c0 = PU(U_FLAGS) & ST_REGEN;
#endif
        // (the tail of the static tile order at several lanes per pixel: only the including kernel that says so — fused.hip.h — every other form keeps its code)
#ifdef RL_FUSED_BODY_TAIL
        constexpr bool kTail = RL_FUSED_BODY_TAIL;
#else
        constexpr bool kTail = false;
#endif
        if (PU(U_FLAGS) & ST_REGEN) raygen_slot<true, decltype(ps), SMP, kTail>(rc, sc, ps, n_samples, n_draws);   // work items from the global dispenser
        RL_T1(0, c0)
#ifdef RL_STAGE_TIMERS
        const bool c1 = PU(U_FLAGS) & ST_RAY;
#endif
        if (PU(U_FLAGS) & ST_RAY) {
            extend_slot(sc, recs, stack, ps);
            RL_T1(1, c1)
            shade_slot<MAT, MEDIUM, LIGHTS, false, SMP>(rc, sc, ps, PU(U_FLAGS), n_vertices, n_draws, n_shadow, n_ext);
        }
        RL_T1(2, c1)
#ifdef RL_STAGE_TIMERS
        const bool c3 = PU(U_FLAGS) & ST_SHADOW;
#endif
        // (the tail form — LDS scene, no medium, not queue-fed — runs the shadow rays of the wave together: leaves enumerated first, triangle tests packed over the lanes;
        // trace.hip.h: occluded_packed.  -DRL_SHADOW_PACKED=0 keeps the per-lane loop there too, for the same-call comparison.  Every other form keeps its code.)
#ifndef RL_SHADOW_PACKED
#define RL_SHADOW_PACKED 1
#endif
        // (exact build only: the tolerance build contracts multiply-adds per call site, so a second site of the triangle test does not repeat the bits of the first,
        // and a frame with a tail must equal the frame without one in either build)
#ifdef RL_FAST_MATH
        constexpr bool kPacked = false;
#else
        constexpr bool kPacked = kTail && RL_SHADOW_PACKED != 0;
#endif
#ifdef RL_STAGE_TIMERS
        PackStats pst;
        if constexpr (kPacked) {
            const bool sh = (PU(U_FLAGS) & ST_SHADOW) != 0u;
            if (__ballot(sh) != 0ull) shadow_slot<true>(sc, recs, stack, ps, sh, stc.pack_cap, &pst);
        } else if (PU(U_FLAGS) & ST_SHADOW) shadow_slot(sc, recs, stack, ps, true, 0, &pst);
#else
        if constexpr (kPacked) {
            const bool sh = (PU(U_FLAGS) & ST_SHADOW) != 0u;
            if (__ballot(sh) != 0ull) shadow_slot<true>(sc, recs, stack, ps, sh, stc.pack_cap);
        } else
        if (PU(U_FLAGS) & ST_SHADOW) shadow_slot(sc, recs, stack, ps);
#endif
#ifdef RL_STAGE_TIMERS
        { const unsigned nsh = (unsigned)__popcll(__ballot(c3)); sh_hist[nsh == 0u ? 0 : 1 + (nsh - 1u) / 16u]++;
          if (nsh) sh_cyc_exec += __builtin_readcyclecounter() - t0;
          if (sh_parity) { const unsigned a = sh_prev, b = nsh; sh_pair[(a == 0u && b == 0u) ? 0 : ((a == 0u || b == 0u) ? 1 : (a + b <= 64u ? 2 : 3))]++; }
          sh_prev = nsh; sh_parity ^= 1u; }
#endif
        RL_T1(3, c3)
#ifdef RL_STAGE_TIMERS
        if (__ballot(c3) != 0ull) {      // loop-level counters of this shadow-stage execution (after the stage's clock reading: not part of its cycles)
            auto wsum = [](unsigned v) { for (int off = 32; off > 0; off >>= 1) v += (unsigned)__shfl_xor((int)v, off, 64); return v; };
            auto wmax = [](unsigned v) { for (int off = 32; off > 0; off >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, off, 64)); return v; };
            sh_loop[0] += wsum(pst.trips_paid); sh_loop[1] += wsum(pst.tests_paid); sh_loop[2] += wmax(pst.lane_trips); sh_loop[3] += wsum(pst.lane_tris);
            sh_loop[4] += wmax(pst.lane_tris); sh_loop[5] += wsum(pst.rounds); sh_loop[6] += wsum(pst.passes);
        }
#endif
    } while (!qmode && !(PU(U_FLAGS) & ST_FINISHED));
    if (!qmode) break;
    }
#ifdef RL_STAGE_TIMERS
    if ((threadIdx.x & 63u) == 0u) { for (int k = 0; k < 4; k++) { atomicAdd(&g_stage_timers[k], tm[k]); atomicAdd(&g_stage_timers[4 + k], ln[k]); } atomicAdd(&g_stage_timers[8], ln[4]);
        for (int k = 0; k < 5; k++) atomicAdd(&g_stage_timers[16 + k], sh_hist[k]); for (int k = 0; k < 4; k++) atomicAdd(&g_stage_timers[21 + k], sh_pair[k]); atomicAdd(&g_stage_timers[25], sh_cyc_exec);
        for (int k = 0; k < 7; k++) atomicAdd(&g_stage_timers[9 + k], sh_loop[k]); }
#endif
    {
        const int which[5] = {STAT_SAMPLES, STAT_VERTICES, STAT_DRAWS, STAT_SHADOW_RAYS, STAT_EXT_RAYS};
        const unsigned vals[5] = {n_samples, n_vertices, n_draws, n_shadow, n_ext};
        block_stats<5>(rc.partials, which, vals);
    }
#ifdef RL_STAGE_TIMERS
    if (threadIdx.x == 0u && blockIdx.x < kFusedWgSlots) { g_fused_wgs[2 * blockIdx.x] = wg_t0; g_fused_wgs[2 * blockIdx.x + 1] = wall_clock64(); }      // (after block_stats' barriers: every wave of the workgroup has ended)
#endif
