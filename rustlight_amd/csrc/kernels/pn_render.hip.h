// pn_render.hip.h — the host side of the point-normal single-scattering integrator (included by wavefront.hip after pplane_render.hip.h; host code only):
// rl_render_point_normal, patterned on render_mc, and render_pn, the one frame sequence it shares with rl_render_point_normal_mis (pnmis_render.hip.h) and
// rl_render_point_normal_taylor (pntaylor_render.hip.h) and rl_render_point_normal_ats (pnats_render.hip.h).
// IntegratorPointNormal: src/integrators/explicit/point_normal.rs:1172-1199, 2584-2633; the kernels are k_pn_pixel and k_pn_chain over the body
// PnPlain<STRATEGY> (pn.hip.h).

// cli.rs:209-224: `-s tr_ex`, AA on (the same with -x, for rl_point_normal_mis_params)
template <typename Params>
static void pn_params_default(Params* params) {
    if (!params) return;
    std::memset(params, 0, sizeof(*params));
    params->spp = 1;
    params->strategy = RL_PN_TR_EX;
    params->use_aa = 1;
    params->stream_mode = RL_STREAM_REFERENCE_ORDER;
    params->shard_index = 0; params->shard_count = 1;
}
extern "C" void rl_point_normal_params_default(rl_point_normal_params* params) { pn_params_default(params); }

// the draws of one camera sample of a constant-count strategy (pn.hip.h's table); 0: the count depends on the data
static unsigned pn_constant_draws(int strategy, bool use_aa) {
    const unsigned aa = use_aa ? 2u : 0u;
    switch (strategy) {
        case RL_PN_TR_EX: return aa + 5u;
        case RL_PN_TR_PHASE: return aa + 3u;
        case RL_PN_EQ_EX: return aa + 5u;
        case RL_PN_EQ_PHASE: return aa + 7u;
        default: return 0u;
    }
}
// ats: rl_render_point_normal_ats, which needs the tree the other kinds refuse
static int check_pn_scene(const rl_context* ctx, bool ats) {
    if (ctx->ds.medium.enabled == 0) { rl_set_error("point-normal needs a medium (add -m; the reference unwraps scene.volume, point_normal.rs:2221)"); return RL_ERR_UNSUPPORTED; }
    if (ats) {
        if (!ctx->surface_emitters_only || ctx->ds.env_emitter >= 0) {
            rl_set_error("point-normal-ats takes surface emitters only (LightSamplerATS::new asserts e.is_surface(), emitter.rs:1292-1294)");
            return RL_ERR_UNSUPPORTED;
        }
        if (ctx->ds.ats_root < 0) { rl_set_error("point-normal-ats needs the light tree (build the scene's emitters with it: -x ats)"); return RL_ERR_UNSUPPORTED; }
        return RL_OK;
    }
    if (ctx->ds.ats_root >= 0) { rl_set_error("point-normal with the light tree (-x ats) is not built"); return RL_ERR_UNSUPPORTED; }
    if (ctx->ds.env_emitter >= 0) { rl_set_error("point-normal does not sample environment emitters"); return RL_ERR_UNSUPPORTED; }
    if (ctx->has_directional) { rl_set_error("point-normal does not take directional lights (their correct_flux is todo!() in the reference, emitter.rs:170-172)"); return RL_ERR_UNSUPPORTED; }
    if (ctx->ds.n_emitters == 0) { rl_set_error("point-normal needs an emitter"); return RL_ERR_NO_EMITTER; }
    return RL_OK;
}

// What tells rl_render_point_normal, rl_render_point_normal_mis and rl_render_point_normal_taylor apart; render_pn below is everything else.
using PnLauncher = void (*)(bool, int, dim3, dim3, size_t, hipStream_t, const RenderConst&, const DeviceScene&, const StackConf&, const PnConst&);
struct PnKind {
    const char* name;                           // "point-normal" | "point-normal-mis" | "point-normal-taylor" | "point-normal-ats", as the error strings say it
    int selector;                               // what the launchers take: the strategy | the family
    unsigned draws;                             // the draws of one camera sample, the jitter's included; 0: the count depends on the data and the chain pass runs
    PnLauncher launch_lds, launch_stream;
    float taylor[8] = {};                       // PnConst::taylor: point-normal-taylor's phase polynomial (pntaylor_render.hip.h); zero for the other kinds
    bool ats = false;                           // point-normal-ats: the scene must carry the light tree, which the other kinds refuse
    const float* ats_angles = nullptr;          // PnConst::ats_angles: point-normal-ats' angles per tree node (pnats_render.hip.h); null for the other kinds
};

// One frame of either kind: the checks, the four sampler modes (PN_MODE_*), the chain pass where the draw count depends on the data, the pixel kernel, and the
// statistics.  counters(totals, stats) turns the kernel's rows into vertices, rng_draws, extension_rays and shadow_rays.
template <typename Params, class Counters>
static int render_pn(rl_context* ctx, const Params* params, const uint64_t* block_seeds, size_t n_blocks, float* out_rgb, rl_render_stats* stats, const PnKind& kind,
                     Counters&& counters) {
    int rcode;
    const std::string name = kind.name;
    if (params->stream_mode == RL_STREAM_STRATIFIED) { rl_set_error(name + " has no stratified sampler (-r stratified is not built)"); return RL_ERR_UNSUPPORTED; }
    if ((rcode = check_streams(params->stream_mode, params->spp, RL_NUMERICS_EXACT, params->shard_index, params->shard_count)) != RL_OK) return rcode;
    if ((rcode = check_pn_scene(ctx, kind.ats)) != RL_OK) return rcode;
    const bool per_sample = params->stream_mode == RL_STREAM_PER_SAMPLE;
    const bool single_pass = !per_sample && ctx->knobs.has(K_REF_SINGLE_PASS);
    const bool chain = !per_sample && !single_pass && kind.draws == 0u;
    const bool advance = !per_sample && !single_pass && kind.draws != 0u;
    if (advance && 256ull * params->spp * kind.draws > 0xffffffffull) {
        rl_set_error(name + ": 256 * spp * D exceeds 2^32 - 1, the reach of the jump a block's stream is entered with (spp = " + std::to_string(params->spp) +
                     ", D = " + std::to_string(kind.draws) + ")");
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
    pc.use_aa = params->use_aa != 0 ? 1 : 0;
    pc.mode = per_sample ? PN_MODE_PER_SAMPLE : single_pass ? PN_MODE_BLOCK : chain ? PN_MODE_GIVEN : PN_MODE_ADVANCE;
    pc.draws = kind.draws;
    pc.pixel_states = ctx->d_sample_states.get();
    std::memcpy(pc.taylor, kind.taylor, sizeof(pc.taylor));
    pc.ats_angles = kind.ats_angles;
    StackConf stc;
    if ((rcode = stack_conf(ctx, n_threads, &stc)) != RL_OK) return rcode;
    const size_t lds = traversal_lds_bytes(ctx, ctx->lds_scene, 256, false);
    if ((rcode = fr.grow_events(4)) != RL_OK) return rcode;
    const hipStream_t st = fr.st;
    const PnLauncher launch = ctx->lds_scene ? kind.launch_lds : kind.launch_stream;
    if (!single_pass && !fr.owned.empty()) hipLaunchKernelGGL(k_seed_pixels, dim3(((unsigned)fr.owned.size() + 63) / 64), dim3(64), 0, st, rc);      // item_seed, item_pixel
    if (chain) {
        RenderConst ra = rc;
        ra.n_items = (unsigned)fr.owned.size(); ra.item_shift = chain_shift;
        if (fr.timing) hipEventRecord(ctx->events[0], st);
        launch(true, kind.selector, dim3(chain_threads / 256), dim3(256), lds, st, ra, ctx->ds, stc, pc);
        if (fr.timing) hipEventRecord(ctx->events[1], st);
    }
    if (fr.timing) hipEventRecord(ctx->events[2], st);
    launch(false, kind.selector, dim3(item_threads / 256), dim3(256), lds, st, rc, ctx->ds, stc, pc);
    if (fr.timing) hipEventRecord(ctx->events[3], st);
    if ((rcode = fr.download()) != RL_OK) return rcode;
    if (stats) {
        counters(fr.totals, stats);
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
// the checks that come before a kind can be told: the frame's arguments and the strategy
template <typename Params>
static int check_pn_params(const rl_context* ctx, const Params* params, const uint64_t* block_seeds, size_t n_blocks, const float* out_rgb) {
    int rcode;
    if ((rcode = check_frame(ctx, params, block_seeds, n_blocks, out_rgb)) != RL_OK) return rcode;
    if (params->strategy < RL_PN_TR_EX || params->strategy > RL_PN_PN_EX) { rl_set_error("strategy must be an rl_pn_strategy (0 .. 6)"); return RL_ERR_INVALID_ARGUMENT; }
    return RL_OK;
}

extern "C" int rl_render_point_normal(rl_context* ctx, const rl_point_normal_params* params, const uint64_t* block_seeds, size_t n_blocks, float* out_rgb,
                                      rl_render_stats* stats) {
    int rcode;
    if ((rcode = check_pn_params(ctx, params, block_seeds, n_blocks, out_rgb)) != RL_OK) return rcode;
    const int strategy = params->strategy;
    const bool use_aa = params->use_aa != 0;
    const unsigned draws = pn_constant_draws(strategy, use_aa);
    const PnKind kind{"point-normal", strategy, draws, launch_pn_lds, launch_pn_stream};
    // the kernel's three rows (pn.hip.h) to the counters
    return render_pn(ctx, params, block_seeds, n_blocks, out_rgb, stats, kind, [&](const unsigned long long* totals, rl_render_stats* s) {
        const bool tr = strategy == RL_PN_TR_EX || strategy == RL_PN_TR_PHASE;
        const bool phase = strategy == RL_PN_TR_PHASE || strategy == RL_PN_EQ_PHASE || strategy == RL_PN_EQ_CLAMPED_PHASE;
        const uint64_t samples = totals[STAT_SAMPLES];
        const uint64_t with_sampler = tr ? samples : totals[STAT_VERTICES];
        s->vertices = with_sampler;
        s->rng_draws = draws ? samples * draws : samples * (use_aa ? 6u : 4u) + with_sampler * (phase ? 3u : 1u);
        s->extension_rays = samples + (phase ? totals[STAT_EXT_RAYS] : 0u);
        s->shadow_rays = phase ? 0u : totals[STAT_SHADOW_RAYS];
    });
}
