// pnats_render.hip.h — the host side of the point-normal integrator over the light tree (included by wavefront.hip after pntaylor_render.hip.h; host code
// only): rl_render_point_normal_ats, which is pn_render.hip.h's render_pn on a scene that carries the tree, with the tree's angles uploaded on first use, the
// light tree's launchers and the counters of a pick of three draws.  The kernels are k_pn_pixel and k_pn_chain over the body PnAts<FAMILY, STRATEGY>
// (pnats.hip.h).

extern "C" void rl_point_normal_ats_params_default(rl_point_normal_ats_params* params) {
    pn_params_default(params);
    if (params) { params->family = RL_PN_ATS_PLAIN; params->strategy = RL_PN_EQ_EX; }
}

// [node][2] theta_o, theta_e of the host tree's LightBounds, beside ds.ats_nodes: LightNode keeps their cosines, importance_ray reads the angles
static int ensure_ats_angles(rl_context* ctx) {
    if (ctx->d_ats_angles || ctx->ds.ats_root < 0) return RL_OK;
    HIP_OK(hipSetDevice(ctx->device));
    return upload(ctx, ctx->ats_angles, &ctx->d_ats_angles);
}

extern "C" int rl_render_point_normal_ats(rl_context* ctx, const rl_point_normal_ats_params* params, const uint64_t* block_seeds, size_t n_blocks, float* out_rgb,
                                          rl_render_stats* stats) {
    int rcode;
    if ((rcode = check_frame(ctx, params, block_seeds, n_blocks, out_rgb)) != RL_OK) return rcode;
    if (params->family != RL_PN_ATS_PLAIN && params->family != RL_PN_ATS_TAYLOR) { rl_set_error("family must be an rl_pn_ats_family (0, 1)"); return RL_ERR_INVALID_ARGUMENT; }
    const bool taylor_family = params->family == RL_PN_ATS_TAYLOR;
    if (!taylor_family && (params->strategy < RL_PN_TR_EX || params->strategy > RL_PN_PN_EX)) { rl_set_error("strategy must be an rl_pn_strategy (0 .. 6)"); return RL_ERR_INVALID_ARGUMENT; }
    if (taylor_family && (params->strategy < RL_PN_TAYLOR_EQ_PHASE || params->strategy > RL_PN_TAYLOR_PN_PHASE)) {
        rl_set_error("strategy must be an rl_pn_taylor_strategy (0 .. 5)");
        return RL_ERR_INVALID_ARGUMENT;
    }
    const int strategy = params->strategy;
    const bool use_aa = params->use_aa != 0;
    const unsigned aa = use_aa ? 2u : 0u;
    PnKind kind{"point-normal-ats", 8 * params->family + strategy, 0u, launch_pnats_lds, launch_pnats_stream};
    kind.ats = true;
    if ((rcode = ensure_ats_angles(ctx)) != RL_OK) return rcode;
    kind.ats_angles = ctx->d_ats_angles;
    if (taylor_family) {
        // the Taylor names as rl_render_point_normal_taylor takes them (pntaylor_render.hip.h): the Isotropic forward, the g = 0 refusal, the phase polynomial
        const bool phase_poly = strategy == RL_PN_TAYLOR_EQ_PHASE || strategy == RL_PN_TAYLOR_EQ_CLAMPED_PHASE || strategy == RL_PN_TAYLOR_PN_PHASE;
        const bool isotropic = ctx->ds.medium.phase == 0;
        const float g = isotropic ? 0.0f : ctx->ds.medium.g;
        if (phase_poly && isotropic && strategy != RL_PN_TAYLOR_PN_PHASE && ctx->ds.medium.enabled != 0) {
            rl_point_normal_ats_params plain = *params;
            plain.family = RL_PN_ATS_PLAIN;
            plain.strategy = strategy == RL_PN_TAYLOR_EQ_PHASE ? RL_PN_EQ_EX : RL_PN_EQ_CLAMPED_EX;
            return rl_render_point_normal_ats(ctx, &plain, block_seeds, n_blocks, out_rgb, stats);
        }
        if (strategy == RL_PN_TAYLOR_PN_PHASE && ctx->ds.medium.enabled != 0 && g == 0.0f) {
            rl_set_error("point-normal-ats: pn_phase_taylor_ex needs a Henyey-Greenstein medium with g != 0 (assert!(g != 0.0), point_normal.rs:1414)");
            return RL_ERR_UNSUPPORTED;
        }
        if (phase_poly) pntaylor_phase_poly(g, kind.taylor);
        // the kernel's three rows (pntaylor.hip.h) to the counters: three emitter draws, one more behind a sampler
        return render_pn(ctx, params, block_seeds, n_blocks, out_rgb, stats, kind, [&](const unsigned long long* totals, rl_render_stats* s) {
            s->vertices = totals[STAT_VERTICES];
            s->rng_draws = totals[STAT_SAMPLES] * (aa + 3u) + totals[STAT_VERTICES];
            s->extension_rays = totals[STAT_SAMPLES];
            s->shadow_rays = totals[STAT_SHADOW_RAYS];
        });
    }
    // the draws of one camera sample of a constant-count strategy (pnats.hip.h's table); 0: the count depends on the data
    const unsigned draws = strategy == RL_PN_TR_EX || strategy == RL_PN_EQ_EX ? aa + 4u : strategy == RL_PN_TR_PHASE ? aa + 3u : strategy == RL_PN_EQ_PHASE ? aa + 6u : 0u;
    kind.draws = draws;
    // the kernel's three rows (pn.hip.h) to the counters
    return render_pn(ctx, params, block_seeds, n_blocks, out_rgb, stats, kind, [&](const unsigned long long* totals, rl_render_stats* s) {
        const bool tr = strategy == RL_PN_TR_EX || strategy == RL_PN_TR_PHASE;
        const bool phase = strategy == RL_PN_TR_PHASE || strategy == RL_PN_EQ_PHASE || strategy == RL_PN_EQ_CLAMPED_PHASE;
        const uint64_t samples = totals[STAT_SAMPLES];
        const uint64_t with_sampler = tr ? samples : totals[STAT_VERTICES];
        s->vertices = with_sampler;
        s->rng_draws = draws ? samples * draws : samples * (aa + 3u) + with_sampler * (phase ? 3u : 1u);
        s->extension_rays = samples + (phase ? totals[STAT_EXT_RAYS] : 0u);
        s->shadow_rays = phase ? 0u : totals[STAT_SHADOW_RAYS];
    });
}
