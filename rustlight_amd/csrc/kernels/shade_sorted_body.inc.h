// shade_sorted_body.inc.h — the body of k_shade_sorted / k_shade_sorted_strat (shade_sorted.hip.h), included inside the kernel: the kernel defines
// `SMP` (the sampler, sampler.hip.h), MEDIUM and CHUNKS, and takes (RenderConst rc, DeviceScene sc, Pool pool).  (Text included, not a function called: an
// inlined device function with the same statements allocates the kernel's registers differently.)
    __shared__ unsigned s_list[256 * CHUNKS];
    __shared__ unsigned s_cnt[kNumBins][CHUNKS][4];
    unsigned n_vertices = 0, n_draws = 0, n_shadow = 0, n_ext = 0;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned slot[CHUNKS], rank[CHUNKS];
    int bin[CHUNKS];
#pragma unroll
    for (unsigned c = 0; c < CHUNKS; c++) {
        slot[c] = (blockIdx.x * CHUNKS + c) * blockDim.x + threadIdx.x;
        const unsigned flags = slot[c] < pool.P ? pool.u[(size_t)U_FLAGS * pool.P + slot[c]] : 0u;
        bin[c] = -1;
        if (flags & ST_RAY) {
            const int prim = (int)pool.u[(size_t)U_PRIM * pool.P + slot[c]];
            bin[c] = 0;
            if (prim >= 0) bin[c] = sc.materials[sc.meshes[sc.tris[prim].mesh].material].type;
        }
        rank[c] = 0;
#pragma unroll
        for (int b = 0; b < kNumBins; b++) {
            const unsigned long long mask = __ballot(bin[c] == b);
            if (bin[c] == b) rank[c] = __popcll(mask & ((1ull << lane) - 1ull));
            if (lane == 0u) s_cnt[b][c][wave] = (unsigned)__popcll(mask);
        }
    }
    __syncthreads();
    unsigned bin_begin[kNumBins + 1];
    unsigned my_off[CHUNKS];
    unsigned run = 0;
#pragma unroll
    for (int b = 0; b < kNumBins; b++) {
        bin_begin[b] = run;
#pragma unroll
        for (unsigned c = 0; c < CHUNKS; c++)
#pragma unroll
            for (unsigned w = 0; w < 4u; w++) { if (b == bin[c] && w == wave) my_off[c] = run; run += s_cnt[b][c][w]; }
    }
    bin_begin[kNumBins] = run;
#pragma unroll
    for (unsigned c = 0; c < CHUNKS; c++) if (bin[c] >= 0) s_list[my_off[c] + rank[c]] = slot[c];
    __syncthreads();
#define RL_SHADE_BIN(B)                                                                                       \
    { const unsigned n = bin_begin[(B) + 1] - bin_begin[B];                                                   \
      for (unsigned i = threadIdx.x; i < n; i += blockDim.x) { PoolState pb{pool, s_list[bin_begin[B] + i]};    \
          shade_slot<B, MEDIUM, LIGHTS_ANY, false, SMP>(rc, sc, pb, pb.u(U_FLAGS), n_vertices, n_draws, n_shadow, n_ext); } }
    RL_SHADE_BIN(0) RL_SHADE_BIN(1) RL_SHADE_BIN(2) RL_SHADE_BIN(3) RL_SHADE_BIN(4)
#undef RL_SHADE_BIN
    {
        const int which[4] = {STAT_VERTICES, STAT_DRAWS, STAT_SHADOW_RAYS, STAT_EXT_RAYS};
        const unsigned vals[4] = {n_vertices, n_draws, n_shadow, n_ext};
        block_stats<4>(rc.partials, which, vals);
    }
