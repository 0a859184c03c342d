// pnmis_render.hip.h — the host side of the point-normal integrator's MIS estimators (included by wavefront.hip after pn_render.hip.h; host code only):
// rl_render_point_normal_mis, patterned on rl_render_point_normal, whose scene checks it shares.  IntegratorPointNormal with use_mis:
// src/integrators/explicit/point_normal.rs:2605-2612, compute_multiple_tr (:2095-2206), compute_multiple_equiangular (:1849-2091), compute_multiple_strategy
// (:1560-1847); the kernels are k_pnmis_pixel and k_pnmis_chain (pnmis.hip.h).

// cli.rs:209-224 with -x: `-s tr_ex`, AA on
extern "C" void rl_point_normal_mis_params_default(rl_point_normal_mis_params* params) {
    if (!params) return;
    std::memset(params, 0, sizeof(*params));
    params->spp = 1;
    params->strategy = RL_PN_TR_EX;
    params->use_aa = 1;
    params->stream_mode = RL_STREAM_REFERENCE_ORDER;
    params->shard_index = 0; params->shard_count = 1;
}

// the distance family of a strategy, pnmis.hip.h's PNMIS_*: the EX / PHASE bit is ignored under MIS
static int pnmis_family_of(int strategy) {
    switch (strategy) {
        case RL_PN_TR_EX: case RL_PN_TR_PHASE: return 0;
        case RL_PN_EQ_EX: case RL_PN_EQ_PHASE: return 1;
        case RL_PN_EQ_CLAMPED_EX: case RL_PN_EQ_CLAMPED_PHASE: return 2;
        default: return 3;
    }
}

extern "C" int rl_render_point_normal_mis(rl_context* ctx, const rl_point_normal_mis_params* params, const uint64_t* block_seeds, size_t n_blocks, float* out_rgb,
                                          rl_render_stats* stats) {
    int rcode;
    if ((rcode = check_frame(ctx, params, block_seeds, n_blocks, out_rgb)) != RL_OK) return rcode;
    if (params->strategy < RL_PN_TR_EX || params->strategy > RL_PN_PN_EX) { rl_set_error("strategy must be an rl_pn_strategy (0 .. 6)"); return RL_ERR_INVALID_ARGUMENT; }
    if (params->stream_mode == RL_STREAM_STRATIFIED) { rl_set_error("point-normal-mis has no stratified sampler (-r stratified is not built)"); return RL_ERR_UNSUPPORTED; }
    if ((rcode = check_streams(params->stream_mode, params->spp, RL_NUMERICS_EXACT, params->shard_index, params->shard_count)) != RL_OK) return rcode;
    if ((rcode = check_pn_scene(ctx)) != RL_OK) return rcode;
    const int family = pnmis_family_of(params->strategy);
    const bool use_aa = params->use_aa != 0;
    const bool per_sample = params->stream_mode == RL_STREAM_PER_SAMPLE;
    const bool single_pass = !per_sample && ctx->knobs.has(K_REF_SINGLE_PASS);
    // the draws of one camera sample (pnmis.hip.h's table); clamped and pn take one more when their third sampler is Some
    const unsigned base_draws = (use_aa ? 2u : 0u) + (family == 0 ? 7u : 8u);
    const bool constant = family < 2;
    const bool chain = !per_sample && !single_pass && !constant;
    const bool advance = !per_sample && !single_pass && constant;
    if (advance && 256ull * params->spp * base_draws > 0xffffffffull) {
        rl_set_error("point-normal-mis: 256 * spp * D exceeds 2^32 - 1, the reach of the jump a block's stream is entered with (spp = " + std::to_string(params->spp) +
                     ", D = " + std::to_string(base_draws) + ")");
        return RL_ERR_UNSUPPORTED;
    }
    HIP_OK(hipSetDevice(ctx->device));
    RenderFrame fr(ctx, block_seeds, n_blocks, out_rgb, 0, nullptr, stats, params->shard_index, params->shard_count);
    const unsigned n_items = single_pass ? (unsigned)fr.owned.size() : fr.n_pixels;
    unsigned chain_shift = 0;
    if (chain) {
        while (chain_shift < 6u && (fr.owned.size() << (chain_shift + 1u)) <= (size_t)fr.cus * 4u * 256u) chain_shift++;
        if (fr.knobs.has(K_ITEM_SHIFT)) chain_shift = std::min(6u, (unsigned)std::max<long long>(0, fr.knobs.i(K_ITEM_SHIFT, 0)));
    }
    const unsigned chain_threads = chain ? std::max(256u, (unsigned)((((size_t)fr.owned.size() << chain_shift) + 255u) / 256u * 256u)) : 0u;
    const unsigned item_threads = std::max(256u, (n_items + 255u) / 256u * 256u);
    const unsigned n_threads = std::max(chain_threads, item_threads);
    if ((rcode = fr.alloc_tables()) != RL_OK) return rcode;
    if ((rcode = ctx->d_item_seed.ensure(fr.n_pixels)) != RL_OK || (rcode = ctx->d_item_pixel.ensure(fr.n_pixels)) != RL_OK) return rcode;
    // [pixel item][4] u64: where a lane's sampler lives between two samples, and what the chain pass hands over (32 bytes per pixel)
    if ((rcode = ctx->d_sample_states.ensure((size_t)std::max(fr.n_pixels, 1u) * 4)) != RL_OK) return rcode;
    if ((rcode = fr.alloc_output(n_threads / 256)) != RL_OK) return rcode;
    if ((rcode = fr.upload(true, true)) != RL_OK || (rcode = fr.zero_rows()) != RL_OK) return rcode;
    RenderConst rc = fr.render_const(params->spp, params->stream_mode, params->seed_variant);
    rc.n_items = n_items;
    rc.split = 1;
    PnConst pc{};
    pc.use_aa = use_aa ? 1 : 0;
    pc.mode = per_sample ? PN_MODE_PER_SAMPLE : single_pass ? PN_MODE_BLOCK : chain ? PN_MODE_GIVEN : PN_MODE_ADVANCE;
    pc.draws = constant ? base_draws : 0u;
    pc.pixel_states = ctx->d_sample_states.get();
    StackConf stc;
    if ((rcode = stack_conf(ctx, n_threads, &stc)) != RL_OK) return rcode;
    const size_t lds = traversal_lds_bytes(ctx, ctx->lds_scene, 256, false);
    if ((rcode = fr.grow_events(4)) != RL_OK) return rcode;
    const hipStream_t st = fr.st;
    const auto launch = ctx->lds_scene ? launch_pnmis_lds : launch_pnmis_stream;
    if (!single_pass && !fr.owned.empty()) hipLaunchKernelGGL(k_seed_pixels, dim3(((unsigned)fr.owned.size() + 63) / 64), dim3(64), 0, st, rc);      // item_seed, item_pixel
    if (chain) {
        RenderConst ra = rc;
        ra.n_items = (unsigned)fr.owned.size(); ra.item_shift = chain_shift;
        if (fr.timing) hipEventRecord(ctx->events[0], st);
        launch(true, family, dim3(chain_threads / 256), dim3(256), lds, st, ra, ctx->ds, stc, pc);
        if (fr.timing) hipEventRecord(ctx->events[1], st);
    }
    if (fr.timing) hipEventRecord(ctx->events[2], st);
    launch(false, family, dim3(item_threads / 256), dim3(256), lds, st, rc, ctx->ds, stc, pc);
    if (fr.timing) hipEventRecord(ctx->events[3], st);
    if ((rcode = fr.download()) != RL_OK) return rcode;
    if (stats) {
        // the kernel's four rows (pnmis.hip.h) to the five counters
        const uint64_t samples = fr.totals[STAT_SAMPLES];
        stats->vertices = fr.totals[STAT_VERTICES];
        stats->rng_draws = samples * base_draws + (constant ? 0u : fr.totals[STAT_VERTICES]);
        stats->extension_rays = samples + fr.totals[STAT_EXT_RAYS];
        stats->shadow_rays = fr.totals[STAT_SHADOW_RAYS];
        stats->iterations = 1; stats->kernel_launches = single_pass ? 1 : (chain ? 3 : 2);
        if (fr.timing) {
            float t = 0.0f;
            if (hipEventElapsedTime(&t, ctx->events[2], ctx->events[3]) == hipSuccess) stats->ms_other = t;
            if (chain && hipEventElapsedTime(&t, ctx->events[0], ctx->events[1]) == hipSuccess) stats->ms_prepass = t;
            (void)hipGetLastError();
        }
    }
    return RL_OK;
}
