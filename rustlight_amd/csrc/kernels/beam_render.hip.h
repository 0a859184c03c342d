// beam_render.hip.h — the host side of the photon beams (included by wavefront.hip after gather_render.hip.h; host code only): the beam pass (rl_beam_generate,
// rl_beam_generate_paths: the light-pass sequences of rl_vpl_generate / rl_vpl_generate_paths over k_beam_generate / k_beam_shoot, beamgen.hip.h), the beam map
// (rl_beam_map_*: split and tree on the host, host/beamtree.cpp, uploaded in the gather's node format) and rl_render_beams, which goes through render_gather
// with k_beam_gather (beam.hip.h).  IntegratorVolPrimitives with primitives = Beams: src/integrators/explicit/vol_primitives.rs:101-199, 437-523, 608-790.

struct rl_beam_set {
    const rl_context* ctx;            // the context that made it (compared, never dereferenced)
    int device;
    HipBuffer<unsigned> words;        // [n_beams][RL_BEAM_WORDS]
    uint64_t n_beams = 0, n_paths = 0;
};
struct rl_beam_map {
    const rl_context* ctx;
    int device;
    HipBuffer<float4> nodes;          // [n_nodes][2]
    HipBuffer<float4> beams;          // [n_sub][3], in leaf order
    uint64_t n_beams = 0, n_sub = 0, n_nodes = 0, n_paths = 0;
    float radius = 0.0f;
};
static const LightPassKind kBeamPass{RL_BEAM_WORDS, "photon-beams: fewer than nb_primitive beams stored within RL_VPL_MAX_PATHS light paths"};
static int check_beam_scene(const rl_context* ctx) {
    if (ctx->ds.medium.enabled == 0) { rl_set_error("photon beams need a medium (add -m; the reference panics, vol_primitives.rs:575)"); return RL_ERR_UNSUPPORTED; }
    return RL_OK;
}
// what both generation entry points refuse before any kernel runs: what rl_vpl_generate(RL_VPL_VOLUME) refuses, with its codes
static int check_beam_generate(const rl_context* ctx, const rl_path_params* params, uint32_t nb_primitive, const rl_sampler* sampler, rl_beam_set** out) {
    if (!ctx || !params || !sampler || !out) return RL_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (nb_primitive == 0 || nb_primitive > (uint32_t)RL_BEAM_MAX) { rl_set_error("nb_primitive must be 1 .. RL_BEAM_MAX"); return RL_ERR_INVALID_ARGUMENT; }
    if (params->has_max_depth && params->max_depth <= 1) { rl_set_error("photon beams need max_depth >= 2 (the light vertex has no edge otherwise)"); return RL_ERR_INVALID_ARGUMENT; }
    int rcode;
    if ((rcode = check_vpl_scene(ctx)) != RL_OK || (rcode = check_beam_scene(ctx)) != RL_OK) return rcode;
    if (ctx->has_directional) { rl_set_error("photon beams do not take a directional light (with a medium the light paths of vpl refuse it)"); return RL_ERR_UNSUPPORTED; }
    return RL_OK;
}
extern "C" int rl_beam_generate(rl_context* ctx, const rl_path_params* params, uint32_t nb_primitive, rl_sampler* sampler, rl_beam_set** out, rl_render_stats* stats) {
    int rcode;
    if ((rcode = check_beam_generate(ctx, params, nb_primitive, sampler, out)) != RL_OK) return rcode;
    HIP_OK(hipSetDevice(ctx->device));
    auto set = std::make_unique<rl_beam_set>();
    set->ctx = ctx; set->device = ctx->device;
    if ((rcode = light_pass_serial(ctx, params, nb_primitive, RL_VPL_ALL, kBeamPass, sampler, &set->words, &set->n_beams, &set->n_paths, stats,
                                   [&](size_t lds, const RenderConst& rc, const StackConf& stc, const VplConst& vc) {
            (ctx->lds_scene ? launch_beamgen_lds : launch_beamgen_stream)(0, ctx->single_bsdf ? ctx->bsdf_type : -1, dim3(1), dim3(256), lds, ctx->stream, rc, ctx->ds, stc, vc, VplPathsConst{});
        })) != RL_OK) return rcode;
    *out = set.release();
    return RL_OK;
}
extern "C" int rl_beam_generate_paths(rl_context* ctx, const rl_path_params* params, uint32_t nb_primitive, rl_sampler* sampler, rl_beam_set** out, rl_render_stats* stats) {
    int rcode;
    if ((rcode = check_beam_generate(ctx, params, nb_primitive, sampler, out)) != RL_OK) return rcode;
    HIP_OK(hipSetDevice(ctx->device));
    auto set = std::make_unique<rl_beam_set>();
    set->ctx = ctx; set->device = ctx->device;
    if ((rcode = light_pass_paths(ctx, params, nb_primitive, RL_VPL_ALL, kBeamPass, sampler, &set->words, &set->n_beams, &set->n_paths, stats,
                                  [&](bool write, unsigned groups, size_t lds, const RenderConst& rc, const StackConf& stc, const VplPathsConst& pc) {
            (ctx->lds_scene ? launch_beamgen_lds : launch_beamgen_stream)(write ? 2 : 1, ctx->single_bsdf ? ctx->bsdf_type : -1, dim3(groups), dim3(256), lds, ctx->stream, rc, ctx->ds, stc,
                                                                          VplConst{}, pc);
        })) != RL_OK) return rcode;
    *out = set.release();
    return RL_OK;
}
extern "C" int rl_beam_info(const rl_beam_set* set, uint64_t* n_beams, uint64_t* n_paths) {
    if (!set) return RL_ERR_INVALID_ARGUMENT;
    if (n_beams) *n_beams = set->n_beams;
    if (n_paths) *n_paths = set->n_paths;
    return RL_OK;
}
extern "C" int rl_beam_read(const rl_beam_set* set, uint32_t* words, size_t n_words) {
    if (!set || !words || n_words != set->n_beams * RL_BEAM_WORDS) return RL_ERR_INVALID_ARGUMENT;
    HIP_OK(hipSetDevice(set->device));
    HIP_OK(hipMemcpy(words, set->words.get(), n_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RL_OK;
}
extern "C" void rl_beam_destroy(rl_beam_set* set) {
    if (!set) return;
    (void)hipSetDevice(set->device);
    delete set;
}
extern "C" int rl_beam_map_build_words(rl_context* ctx, const uint32_t* words, size_t n_beams, uint64_t n_paths, float radius, rl_beam_map** out) {
    if (!ctx || !out || (n_beams && !words)) return RL_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int rcode;
    if ((rcode = check_beam_scene(ctx)) != RL_OK || (rcode = check_photon_radius(radius)) != RL_OK) return rcode;
    if (n_paths == 0) { rl_set_error("a beam map needs the number of light paths its beams come from (n_paths >= 1)"); return RL_ERR_INVALID_ARGUMENT; }
    std::vector<uint32_t> sub;
    ElementTree tree;
    if ((rcode = split_beams(words, n_beams, &sub)) != RL_OK) return rcode;
    const size_t n_sub = sub.size() / RL_BEAM_WORDS;
    if ((rcode = build_beam_tree(sub.data(), n_sub, radius, &tree)) != RL_OK) return rcode;
    const std::vector<float4> h_nodes = pack_tree_nodes(tree);
    std::vector<float4> h_beams(3 * n_sub);
    for (size_t i = 0; i < n_sub; i++) {
        float f[RL_BEAM_WORDS];
        std::memcpy(f, &sub[(size_t)tree.order[i] * RL_BEAM_WORDS], sizeof f);       // o, length | d, flags | radiance, path
        h_beams[3 * i] = make_float4(f[0], f[1], f[2], f[3]);
        h_beams[3 * i + 1] = make_float4(f[4], f[5], f[6], 0.0f);
        h_beams[3 * i + 2] = make_float4(f[8], f[9], f[10], 0.0f);
    }
    HIP_OK(hipSetDevice(ctx->device));
    auto map = std::make_unique<rl_beam_map>();
    map->ctx = ctx; map->device = ctx->device;
    if ((rcode = map->nodes.ensure(h_nodes.size())) != RL_OK || (rcode = map->beams.ensure(h_beams.size())) != RL_OK) return rcode;
    HIP_OK(hipMemcpy(map->nodes.get(), h_nodes.data(), h_nodes.size() * sizeof(float4), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(map->beams.get(), h_beams.data(), h_beams.size() * sizeof(float4), hipMemcpyHostToDevice));
    map->n_beams = n_beams; map->n_sub = n_sub; map->n_nodes = tree.n_nodes(); map->n_paths = n_paths; map->radius = radius;
    *out = map.release();
    return RL_OK;
}
extern "C" int rl_beam_map_build(rl_context* ctx, const rl_beam_set* set, float radius, rl_beam_map** out) {
    if (!ctx || !set || !out) return RL_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (set->ctx != ctx) { rl_set_error("the beam set belongs to another context"); return RL_ERR_INVALID_ARGUMENT; }
    HIP_OK(hipSetDevice(ctx->device));
    std::vector<uint32_t> words((size_t)set->n_beams * RL_BEAM_WORDS);
    HIP_OK(hipMemcpy(words.data(), set->words.get(), words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return rl_beam_map_build_words(ctx, words.data(), (size_t)set->n_beams, set->n_paths, radius, out);
}
extern "C" int rl_beam_map_info(const rl_beam_map* map, uint64_t* n_beams, uint64_t* n_sub, uint64_t* n_nodes, uint64_t* n_paths, float* radius) {
    if (!map) return RL_ERR_INVALID_ARGUMENT;
    if (n_beams) *n_beams = map->n_beams;
    if (n_sub) *n_sub = map->n_sub;
    if (n_nodes) *n_nodes = map->n_nodes;
    if (n_paths) *n_paths = map->n_paths;
    if (radius) *radius = map->radius;
    return RL_OK;
}
extern "C" int rl_beam_map_read(const rl_beam_map* map, size_t node_capacity, float* node_boxes, uint32_t* node_links, size_t beam_capacity, float* beams) {
    if (!map || !node_boxes || !node_links || !beams) return RL_ERR_INVALID_ARGUMENT;
    if (node_capacity < map->n_nodes || beam_capacity < map->n_sub) { rl_set_error("rl_beam_map_read: a capacity is too small"); return RL_ERR_INVALID_ARGUMENT; }
    HIP_OK(hipSetDevice(map->device));
    std::vector<float4> h_nodes(2 * (size_t)map->n_nodes);
    HIP_OK(hipMemcpy(h_nodes.data(), map->nodes.get(), h_nodes.size() * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(beams, map->beams.get(), (size_t)map->n_sub * 3 * sizeof(float4), hipMemcpyDeviceToHost));
    unpack_tree_nodes(h_nodes, (size_t)map->n_nodes, node_boxes, node_links);
    return RL_OK;
}
extern "C" void rl_beam_map_destroy(rl_beam_map* map) {
    if (!map) return;
    (void)hipSetDevice(map->device);
    delete map;
}
extern "C" int rl_render_beams(rl_context* ctx, const rl_beam_map* map, uint32_t spp, int32_t seed_variant, uint32_t shard_index, uint32_t shard_count,
                               const uint64_t* block_seeds, size_t n_blocks, float* out_rgb, rl_render_stats* stats) {
    if (!map) return RL_ERR_INVALID_ARGUMENT;
    static const GatherKind kind{"photon-beams", "beam map", check_beam_scene, 1, {STAT_BEAM_ACCEPTED}, {STAT_BEAM_ACCEPTED_HI}};      // reserved[1] = beams accepted
    return render_gather(ctx, kind, map->ctx, spp, seed_variant, shard_index, shard_count, block_seeds, n_blocks, out_rgb, stats,
                         [&](bool lds_scene, dim3 grid, size_t lds, hipStream_t st, const RenderConst& rc, const StackConf& stc) {
        BeamConst bc{};
        bc.nodes = map->nodes.get(); bc.beams = map->beams.get(); bc.n_nodes = (unsigned)map->n_nodes;
        bc.radius2 = map->radius * map->radius;                                 // self.radius * self.radius
        bc.half_inv_radius = 0.5f / map->radius;                                // 0.5 / self.radius
        bc.norm_photon = 1.0f / (float)map->n_paths;                            // 1.0 / nb_path_shot as f32 (vol_primitives.rs:707)
        (lds_scene ? launch_beam_lds : launch_beam_stream)(grid, dim3(256), lds, st, rc, ctx->ds, stc, bc);
    });
}
