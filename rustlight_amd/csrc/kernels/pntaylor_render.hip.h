// pntaylor_render.hip.h — the host side of the point-normal integrator's Taylor strategies (included by wavefront.hip after pnmis_render.hip.h; host code
// only): rl_render_point_normal_taylor, which is pn_render.hip.h's render_pn with the chain pass always on, the Taylor launchers and counters, and the phase
// polynomial of the frame.  The kernels are k_pn_pixel and k_pn_chain over the body PnTaylor<STRATEGY> (pntaylor.hip.h).

extern "C" void rl_point_normal_taylor_params_default(rl_point_normal_taylor_params* params) {
    pn_params_default(params);
    if (params) params->strategy = RL_PN_TAYLOR_EQ_TR;
}

// f32::powi = llvm.powi: __powisf2's order of products (devmath.hip.h's powi_f, on the host)
static float pntaylor_powi(float a, int b) {
    float r = 1.0f;
    for (;;) { if (b & 1) r *= a; b /= 2; if (b == 0) break; a *= a; }
    return r;
}
// Poly6::phase(g) (point_normal_poly.rs:191-215) into out[0..6] and clamp_angle_phase(g) (point_normal.rs:395-399) into out[7]: f32 statement for statement,
// the sums left to right, the literals rounded to f32 (-ffp-contract=off holds for this file too)
static void pntaylor_phase_poly(float g, float out[8]) {
    const auto power = [](float v, int i) { return pntaylor_powi(v, i); };
    const float hterm = 1.0f + g * g;
    const float hterm_sqrt = std::sqrt(hterm);
    const float h_3_2 = 1.0f / (hterm * hterm_sqrt);
    const float h_5_2 = 1.0f / (power(hterm, 2) * hterm_sqrt);
    const float h_7_2 = 1.0f / (power(hterm, 3) * hterm_sqrt);
    const float h_9_2 = 1.0f / (power(hterm, 4) * hterm_sqrt);
    const float h_11_2 = 1.0f / (power(hterm, 5) * hterm_sqrt);
    const float h_13_2 = 1.0f / (power(hterm, 6) * hterm_sqrt);
    const float h_15_2 = 1.0f / (power(hterm, 7) * hterm_sqrt);
    out[0] = h_3_2;
    out[1] = -3.0f * h_5_2 * g;
    out[2] = (15.0f / 2.0f) * h_7_2 * power(g, 2);
    out[3] = 0.5f * (g - 33.0f * power(g, 3) + power(g, 5)) * h_9_2;
    out[4] = -0.625f * (4.0f * power(g, 2) - 55.0f * power(g, 4) + 4.0f * power(g, 6)) * h_11_2;
    out[5] = (-0.025f * g + 8.65f * power(g, 3) - 69.275f * power(g, 5) + 8.65f * power(g, 7) - 0.025f * power(g, 9)) * h_13_2;
    out[6] = (power(g, 2) * (0.3333333333333333f - 24.916666666666664f * power(g, 2) + 137.1875f * power(g, 4) - 24.916666666666664f * power(g, 6) +
                             0.3333333333333333f * power(g, 8))) * h_15_2;
    out[7] = 18.8217f - 93.8831f * g + 184.173f * power(g, 2) - 160.212f * power(g, 3) + 51.7683f * power(g, 4);
}

extern "C" int rl_render_point_normal_taylor(rl_context* ctx, const rl_point_normal_taylor_params* params, const uint64_t* block_seeds, size_t n_blocks,
                                             float* out_rgb, rl_render_stats* stats) {
    int rcode;
    if ((rcode = check_frame(ctx, params, block_seeds, n_blocks, out_rgb)) != RL_OK) return rcode;
    if (params->strategy < RL_PN_TAYLOR_EQ_PHASE || params->strategy > RL_PN_TAYLOR_PN_PHASE) {
        rl_set_error("strategy must be an rl_pn_taylor_strategy (0 .. 5)");
        return RL_ERR_INVALID_ARGUMENT;
    }
    const int strategy = params->strategy;
    const bool phase_poly = strategy == RL_PN_TAYLOR_EQ_PHASE || strategy == RL_PN_TAYLOR_EQ_CLAMPED_PHASE || strategy == RL_PN_TAYLOR_PN_PHASE;
    const bool isotropic = ctx->ds.medium.phase == 0;
    const float g = isotropic ? 0.0f : ctx->ds.medium.g;
    if (phase_poly && isotropic && strategy != RL_PN_TAYLOR_PN_PHASE && ctx->ds.medium.enabled != 0) {
        // PhaseFunction::Isotropic() => Some(Box::new(equiangular)) (:1278): the plain strategy, through its own entry point
        rl_point_normal_params plain;
        std::memcpy(&plain, params, sizeof(plain));
        static_assert(sizeof(rl_point_normal_params) == sizeof(rl_point_normal_taylor_params), "the two structs have the same fields");
        plain.strategy = strategy == RL_PN_TAYLOR_EQ_PHASE ? RL_PN_EQ_EX : RL_PN_EQ_CLAMPED_EX;
        return rl_render_point_normal(ctx, &plain, block_seeds, n_blocks, out_rgb, stats);
    }
    if (strategy == RL_PN_TAYLOR_PN_PHASE && ctx->ds.medium.enabled != 0 && g == 0.0f) {
        rl_set_error("point-normal-taylor: pn_phase_taylor_ex needs a Henyey-Greenstein medium with g != 0 (assert!(g != 0.0), point_normal.rs:1414)");
        return RL_ERR_UNSUPPORTED;
    }
    float taylor[8] = {};
    if (phase_poly) pntaylor_phase_poly(g, taylor);
    const unsigned base_draws = (params->use_aa != 0 ? 2u : 0u) + 4u;
    PnKind kind{"point-normal-taylor", strategy, 0u, launch_pntaylor_lds, launch_pntaylor_stream};
    std::memcpy(kind.taylor, taylor, sizeof(taylor));
    // the kernel's three rows (pntaylor.hip.h) to the counters
    return render_pn(ctx, params, block_seeds, n_blocks, out_rgb, stats, kind, [&](const unsigned long long* totals, rl_render_stats* s) {
        s->vertices = totals[STAT_VERTICES];
        s->rng_draws = totals[STAT_SAMPLES] * base_draws + totals[STAT_VERTICES];
        s->extension_rays = totals[STAT_SAMPLES];
        s->shadow_rays = totals[STAT_SHADOW_RAYS];
    });
}
