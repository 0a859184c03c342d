// vrl_render.hip.h — the host side of the virtual ray lights (included by wavefront.hip after beam_render.hip.h; host code only).  The beams are those of the
// beam pass (rl_beam_generate / rl_beam_generate_paths: the reference's VRL arm calls convert_beams(false, ..) and stops on the same count).  rl_vrl_map_*: the
// partition by from_surface (word 7 bit 0), avg and rr, the surface beams into a BeamHalf (beam_render.hip.h); rl_render_vrl: render_gather's frame around
// two launches, k_vrl_chain and k_vrl_gather (vrl.hip.h).  IntegratorVolPrimitives with primitives = VRL: src/integrators/explicit/vol_primitives.rs:201-253,
// 608-699, 741-764.

struct rl_vrl_map {
    const rl_context* ctx;            // the context that made it (compared, never dereferenced)
    int device;
    BeamHalf half;                    // the surface beams' sub-beams and the beam tree over them
    HipBuffer<float4> vrls;           // [n_vrl][3]: o, length | d, rr | radiance, 0, in storing order
    uint64_t n_surface = 0, n_vrl = 0, n_paths = 0;
    float radius = 0.0f, avg = 0.0f;
};
static int check_vrl_scene(const rl_context* ctx) { return check_medium(ctx, "virtual ray lights"); }
// the worst case of a block's draws, every VRL surviving in every sample: what rng_advance's 32-bit count must hold
static int check_vrl_draws(uint32_t spp, uint64_t n_vrl) {
    if (256ull * spp * (2ull + 3ull * n_vrl) >= (1ull << 32)) {
        rl_set_error("virtual-ray-lights: 256 * spp * (2 + 3 * VRLs) reaches 2^32, the reach of the jumps a block's stream is entered with (spp = " + std::to_string(spp) +
                     ", VRLs = " + std::to_string(n_vrl) + ")");
        return RL_ERR_UNSUPPORTED;
    }
    return RL_OK;
}
extern "C" int rl_vrl_map_build_words(rl_context* ctx, const uint32_t* words, size_t n_beams, uint64_t n_paths, float radius, rl_vrl_map** out) {
    if (!ctx || !out || (n_beams && !words)) return RL_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int rcode;
    if ((rcode = check_vrl_scene(ctx)) != RL_OK || (rcode = check_photon_radius(radius)) != RL_OK) return rcode;
    if (n_paths == 0) { rl_set_error("a VRL map needs the number of light paths its beams come from (n_paths >= 1)"); return RL_ERR_INVALID_ARGUMENT; }
    if (n_beams > (size_t)RL_BEAM_MAX + 4096) { rl_set_error("too many beams"); return RL_ERR_INVALID_ARGUMENT; }
    // beams.into_iter().partition(|b| b.from_surface): both halves keep the storing order
    std::vector<uint32_t> surface;
    std::vector<float4> h_vrls;
    for (size_t i = 0; i < n_beams; i++) {
        const uint32_t* w = words + i * RL_BEAM_WORDS;
        if (w[7] & 1u) { surface.insert(surface.end(), w, w + RL_BEAM_WORDS); continue; }
        float f[RL_BEAM_WORDS];
        std::memcpy(f, w, sizeof f);                                        // o, length | d, flags | radiance, path
        for (int k : {0, 1, 2, 3, 4, 5, 6, 8, 9, 10})
            if (!std::isfinite(f[k])) { rl_set_error("a VRL record has a non-finite o, d, length or radiance"); return RL_ERR_INVALID_ARGUMENT; }
        h_vrls.push_back(make_float4(f[0], f[1], f[2], f[3]));
        h_vrls.push_back(make_float4(f[4], f[5], f[6], 0.0f));
        h_vrls.push_back(make_float4(f[8], f[9], f[10], 0.0f));
    }
    const size_t n_surface = surface.size() / RL_BEAM_WORDS, n_vrl = h_vrls.size() / 3;
    if (n_surface == 0) { rl_set_error("a VRL map needs a surface beam (word 7 bit 0): the split has nothing to average, and a generated set always holds the light's beam"); return RL_ERR_INVALID_ARGUMENT; }
    // avg_vrl_rad = vrl.iter().map(|v| v.radiance.channel_max()).sum::<f32>() / vrl.len() as f32; rr = ((channel_max / avg) * 0.01).min(1.0): f32::min and
    // f32::max return the operand that is no NaN, as fminf / fmaxf do.  No VRL: the sum is 0 / 0 and nothing reads it; it is reported as 0.
    float sum = 0.0f;
    for (size_t i = 0; i < n_vrl; i++) { const float4 r = h_vrls[3 * i + 2]; sum = sum + std::fmax(r.x, std::fmax(r.y, r.z)); }
    const float avg = n_vrl ? sum / (float)n_vrl : 0.0f;
    for (size_t i = 0; i < n_vrl; i++) {
        const float4 r = h_vrls[3 * i + 2];
        h_vrls[3 * i + 1].w = std::fmin((std::fmax(r.x, std::fmax(r.y, r.z)) / avg) * 0.01f, 1.0f);
    }
    // ---- the surface beams: split and beam tree (avg_split over the surface beams alone)
    auto map = new_handle<rl_vrl_map>(ctx);
    BeamHalfHost host;
    if ((rcode = beam_half_build(&map->half, &host, ctx->device, surface.data(), n_surface, radius)) != RL_OK || (rcode = map->vrls.ensure(std::max<size_t>(h_vrls.size(), 1))) != RL_OK) return rcode;
    if (n_vrl) HIP_OK(hipMemcpy(map->vrls.get(), h_vrls.data(), h_vrls.size() * sizeof(float4), hipMemcpyHostToDevice));
    map->n_surface = n_surface; map->n_vrl = n_vrl; map->n_paths = n_paths; map->radius = radius; map->avg = avg;
    *out = map.release();
    return RL_OK;
}
extern "C" int rl_vrl_map_build(rl_context* ctx, const rl_beam_set* set, float radius, rl_vrl_map** out) {
    if (!ctx || !set || !out) return RL_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int rcode;
    std::vector<uint32_t> words;
    if ((rcode = set_words_to_host(ctx, set->ctx, "beam set", set->words, (size_t)set->n_beams * RL_BEAM_WORDS, &words)) != RL_OK) return rcode;
    return rl_vrl_map_build_words(ctx, words.data(), (size_t)set->n_beams, set->n_paths, radius, out);
}
extern "C" int rl_vrl_map_info(const rl_vrl_map* map, uint64_t* n_surface, uint64_t* n_sub, uint64_t* n_nodes, uint64_t* n_vrl, uint64_t* n_paths, float* radius, float* avg) {
    if (!map) return RL_ERR_INVALID_ARGUMENT;
    if (n_surface) *n_surface = map->n_surface;
    if (n_sub) *n_sub = map->half.n_sub;
    if (n_nodes) *n_nodes = map->half.n_nodes;
    if (n_vrl) *n_vrl = map->n_vrl;
    if (n_paths) *n_paths = map->n_paths;
    if (radius) *radius = map->radius;
    if (avg) *avg = map->avg;
    return RL_OK;
}
extern "C" int rl_vrl_map_read(const rl_vrl_map* map, size_t node_capacity, float* node_boxes, uint32_t* node_links, size_t beam_capacity, float* beams, size_t vrl_capacity, float* vrls) {
    if (!map || !node_boxes || !node_links || !beams || (map->n_vrl && !vrls)) return RL_ERR_INVALID_ARGUMENT;
    if (node_capacity < map->half.n_nodes || beam_capacity < map->half.n_sub || vrl_capacity < map->n_vrl) { rl_set_error("rl_vrl_map_read: a capacity is too small"); return RL_ERR_INVALID_ARGUMENT; }
    HIP_OK(hipSetDevice(map->device));
    if (map->n_vrl) HIP_OK(hipMemcpy(vrls, map->vrls.get(), (size_t)map->n_vrl * 3 * sizeof(float4), hipMemcpyDeviceToHost));
    return beam_half_read(map->half, node_boxes, node_links, beams);
}
extern "C" void rl_vrl_map_destroy(rl_vrl_map* map) { destroy_handle(map); }
extern "C" int rl_render_vrl(rl_context* ctx, const rl_vrl_map* map, uint32_t spp, int32_t seed_variant, uint32_t shard_index, uint32_t shard_count,
                             const uint64_t* block_seeds, size_t n_blocks, float* out_rgb, rl_render_stats* stats) {
    if (!map) return RL_ERR_INVALID_ARGUMENT;
    // render_gather's refusals in its order, then the reach of the chained starts; render_gather repeats the first ones
    int rcode;
    if ((rcode = check_frame(ctx, spp, block_seeds, n_blocks, out_rgb)) != RL_OK || (rcode = check_vrl_scene(ctx)) != RL_OK) return rcode;
    if (map->ctx != ctx) { rl_set_error("the VRL map belongs to another context"); return RL_ERR_INVALID_ARGUMENT; }
    if (shard_index >= (shard_count ? shard_count : 1)) return RL_ERR_INVALID_ARGUMENT;
    if (spp > (uint32_t)RL_VPL_MAX_SPP) { rl_set_error("virtual-ray-lights takes at most RL_VPL_MAX_SPP spp (a block's stream is entered with 32-bit jumps)"); return RL_ERR_UNSUPPORTED; }
    if ((rcode = check_vrl_draws(spp, map->n_vrl)) != RL_OK) return rcode;
    HIP_OK(hipSetDevice(ctx->device));
    const size_t n_owned_max = n_blocks / (shard_count ? shard_count : 1) + 1;
    HipBuffer<unsigned> d_starts, d_totals;       // freed once render_gather has synchronised
    if ((rcode = d_starts.ensure(n_owned_max * 256)) != RL_OK || (rcode = d_totals.ensure(n_owned_max)) != RL_OK) return rcode;
    // reserved[1] = beams accepted, [2] = VRLs that passed the roulette, [3] = of those visible; the counters take every statistics row, so the samples are derived
    const GatherKind kind{"virtual-ray-lights", "VRL map", check_vrl_scene, 3, {STAT_PPLANE_BEAMS, STAT_PPLANE_ISECT, STAT_PPLANE_VISIBLE},
                          {STAT_PPLANE_BEAMS_HI, STAT_PPLANE_ISECT_HI, STAT_PPLANE_VISIBLE_HI}, 2, true};
    unsigned n_owned = 0;
    EventPair chain_ev;
    if ((rcode = chain_ev.open(stats != nullptr && !ctx->knobs.has(K_NO_EVENTS))) != RL_OK) return rcode;
    rcode = render_gather(ctx, kind, map->ctx, spp, seed_variant, shard_index, shard_count, block_seeds, n_blocks, out_rgb, stats,
                          [&](bool lds_scene, dim3 grid, size_t lds, hipStream_t st, const RenderConst& rc, const StackConf& stc) {
        VrlConst vc{};
        vc.beam = beam_half_const(map->half, map->radius, map->n_paths);
        vc.vrls = map->vrls.get(); vc.n_vrl = (unsigned)map->n_vrl;
        vc.starts = d_starts.get(); vc.totals = d_totals.get();
        n_owned = grid.x;
        chain_ev.begin(st);
        launch_vrl_chain(st, rc, vc);
        chain_ev.end(st);
        (lds_scene ? launch_vrl_lds : launch_vrl_stream)(grid, dim3(256), lds, st, rc, ctx->ds, stc, vc);
    });
    if (rcode != RL_OK) return rcode;
    if (stats) {
        std::vector<unsigned> totals(n_owned);
        if (n_owned) HIP_OK(hipMemcpy(totals.data(), d_totals.get(), n_owned * sizeof(unsigned), hipMemcpyDeviceToHost));
        uint64_t draws = 0;
        for (unsigned t : totals) draws += t;
        stats->rng_draws = draws;                                               // 2 + n_vrl + 2 A per sample, walked by the chain pass
        stats->shadow_rays = stats->reserved[2];                                // each VRL that passes the roulette takes one visibility ray
        stats->kernel_launches = n_owned > 0 ? 2 : 0;
        chain_ev.add();
        stats->ms_prepass = chain_ev.ms;                                        // the chain pass; ms_other spans both kernels
    }
    return RL_OK;
}
