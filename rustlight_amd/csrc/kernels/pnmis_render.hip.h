// pnmis_render.hip.h — the host side of the point-normal integrator's MIS estimators (included by wavefront.hip after pn_render.hip.h; host code only):
// rl_render_point_normal_mis, which is pn_render.hip.h's render_pn with the family's draw count, launchers and counters.  IntegratorPointNormal with use_mis:
// src/integrators/explicit/point_normal.rs:2605-2612, compute_multiple_tr (:2095-2206), compute_multiple_equiangular (:1849-2091), compute_multiple_strategy
// (:1560-1847); the kernels are k_pn_pixel and k_pn_chain over the body PnMis<FAMILY> (pnmis.hip.h).

extern "C" void rl_point_normal_mis_params_default(rl_point_normal_mis_params* params) { pn_params_default(params); }

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
    if ((rcode = check_pn_params(ctx, params, block_seeds, n_blocks, out_rgb)) != RL_OK) return rcode;
    const int family = pnmis_family_of(params->strategy);
    // the draws of one camera sample (pnmis.hip.h's table); clamped and pn take one more when their third sampler is Some
    const unsigned base_draws = (params->use_aa != 0 ? 2u : 0u) + (family == 0 ? 7u : 8u);
    const bool constant = family < 2;
    const PnKind kind{"point-normal-mis", family, constant ? base_draws : 0u, launch_pnmis_lds, launch_pnmis_stream};
    // the kernel's four rows (pnmis.hip.h) to the counters
    return render_pn(ctx, params, block_seeds, n_blocks, out_rgb, stats, kind, [&](const unsigned long long* totals, rl_render_stats* s) {
        s->vertices = totals[STAT_VERTICES];
        s->rng_draws = totals[STAT_SAMPLES] * base_draws + (constant ? 0u : totals[STAT_VERTICES]);
        s->extension_rays = totals[STAT_SAMPLES] + totals[STAT_EXT_RAYS];
        s->shadow_rays = totals[STAT_SHADOW_RAYS];
    });
}
