// beam_render.hip.h — the host side of the photon beams (included by wavefront.hip after gather_render.hip.h; host code only): the beam pass (rl_beam_generate,
// rl_beam_generate_paths: the light-pass sequences of rl_vpl_generate / rl_vpl_generate_paths over k_beam_generate / k_beam_shoot, beamgen.hip.h), the beam map
// (rl_beam_map_*: split and tree on the host, host/beamtree.cpp, uploaded in the gather's node format) and rl_render_beams, which goes through render_gather
// with k_beam_gather (beam.hip.h).  IntegratorVolPrimitives with primitives = Beams: src/integrators/explicit/vol_primitives.rs:101-199, 437-523, 608-790.
// What the beam pass shares with the virtual ray lights and the photon planes (vrl_render.hip.h, pplane_render.hip.h) is written here once: BeamHalf, the split
// beams and their tree as all three maps hold them; light_pass, either light-pass sequence behind one launch; check_medium, set_words_to_host, new_handle.

struct rl_beam_set {
    const rl_context* ctx;            // the context that made it (compared, never dereferenced)
    int device;
    HipBuffer<unsigned> words;        // [n_beams][RL_BEAM_WORDS]
    uint64_t n_beams = 0, n_paths = 0;
};
// The beam half of a map: the sub-beams of the beams a map was given and the beam tree over them, in the gather's formats (launch.h: BeamConst)
struct __attribute__((visibility("hidden"))) BeamHalf {      // (host-internal: not a symbol of the library)
    HipBuffer<float4> nodes;          // [n_nodes][2]
    HipBuffer<float4> beams;          // [n_sub][3], in leaf order
    uint64_t n_sub = 0, n_nodes = 0;
};
// The host side of one build.  The caller owns it, so that it is freed when the caller's map is complete and not in the middle of its build: a photon-plane map
// builds its plane tree after the beam half, and returning these ten or so megabytes to the heap before that made every second build 14 ms slower
// (profiles/beam_pass_host_note.md).
struct __attribute__((visibility("hidden"))) BeamHalfHost {
    std::vector<uint32_t> sub;
    ElementTree tree;
    std::vector<float4> h_nodes, h_beams;
};
// split and tree on the host (host/beamtree.cpp), then the upload to `device`
static int beam_half_build(BeamHalf* half, BeamHalfHost* host, int device, const uint32_t* words, size_t n_beams, float radius) {
    int rcode;
    std::vector<uint32_t>& sub = host->sub;
    ElementTree& tree = host->tree;
    std::vector<float4>& h_nodes = host->h_nodes;
    std::vector<float4>& h_beams = host->h_beams;
    if ((rcode = split_beams(words, n_beams, &sub)) != RL_OK) return rcode;
    const size_t n_sub = sub.size() / RL_BEAM_WORDS;
    if ((rcode = build_beam_tree(sub.data(), n_sub, radius, &tree)) != RL_OK) return rcode;
    h_nodes = pack_tree_nodes(tree);
    h_beams = std::vector<float4>(3 * n_sub);
    for (size_t i = 0; i < n_sub; i++) {
        float f[RL_BEAM_WORDS];
        std::memcpy(f, &sub[(size_t)tree.order[i] * RL_BEAM_WORDS], sizeof f);       // o, length | d, flags | radiance, path
        h_beams[3 * i] = make_float4(f[0], f[1], f[2], f[3]);
        h_beams[3 * i + 1] = make_float4(f[4], f[5], f[6], 0.0f);
        h_beams[3 * i + 2] = make_float4(f[8], f[9], f[10], 0.0f);
    }
    HIP_OK(hipSetDevice(device));
    if ((rcode = upload_tree(h_nodes, h_beams, &half->nodes, &half->beams)) != RL_OK) return rcode;
    half->n_sub = n_sub; half->n_nodes = tree.n_nodes();
    return RL_OK;
}
static BeamConst beam_half_const(const BeamHalf& half, float radius, uint64_t n_paths) {
    BeamConst bc{};
    bc.nodes = half.nodes.get(); bc.beams = half.beams.get(); bc.n_nodes = (unsigned)half.n_nodes;
    bc.radius2 = radius * radius;                                               // self.radius * self.radius
    bc.half_inv_radius = 0.5f / radius;                                         // 0.5 / self.radius
    bc.norm_photon = 1.0f / (float)n_paths;                                     // 1.0 / nb_path_shot as f32 (vol_primitives.rs:707)
    return bc;
}
static int beam_half_read(const BeamHalf& half, float* node_boxes, uint32_t* node_links, float* beams) {
    return read_tree(half.nodes, (size_t)half.n_nodes, half.beams, (size_t)half.n_sub * 3, node_boxes, node_links, beams);
}
struct rl_beam_map {
    const rl_context* ctx;
    int device;
    BeamHalf half;
    uint64_t n_beams = 0, n_paths = 0;
    float radius = 0.0f;
};
static const LightPassKind kBeamPass{RL_BEAM_WORDS, "photon-beams: fewer than nb_primitive beams stored within RL_VPL_MAX_PATHS light paths"};
// a set or a map of `ctx`, on its device
template <class T>
static std::unique_ptr<T> new_handle(rl_context* ctx) {
    auto h = std::make_unique<T>();
    h->ctx = ctx; h->device = ctx->device;
    return h;
}
// what the beam, VRL and plane entry points refuse without a medium; `who` is the integrator's primitives in the plural
static int check_medium(const rl_context* ctx, const char* who) {
    if (ctx->ds.medium.enabled == 0) { rl_set_error(std::string(who) + " need a medium (add -m; the reference panics, vol_primitives.rs:575)"); return RL_ERR_UNSUPPORTED; }
    return RL_OK;
}
static int check_beam_scene(const rl_context* ctx) { return check_medium(ctx, "photon beams"); }
// a map build from a set: the set (`what`) is this context's, and its `n_words` words come to the host
static int set_words_to_host(const rl_context* ctx, const rl_context* set_ctx, const char* what, const HipBuffer<unsigned>& d_words, size_t n_words, std::vector<uint32_t>* words) {
    if (set_ctx != ctx) { rl_set_error(std::string("the ") + what + " belongs to another context"); return RL_ERR_INVALID_ARGUMENT; }
    HIP_OK(hipSetDevice(ctx->device));
    words->resize(n_words);
    HIP_OK(hipMemcpy(words->data(), d_words.get(), n_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RL_OK;
}
// Either light-pass sequence over one kernel family: light_pass_serial, or (per_path) light_pass_paths.  shoot(which, groups, lds_bytes, rc, stc, vc, pc)
// launches which = 0 the serial lane, 1 the count pass, 2 the write pass; the constants its sequence does not fill are empty.
template <class Shoot>
static int light_pass(bool per_path, rl_context* ctx, const rl_path_params* params, uint32_t nb_primitive, const LightPassKind& kind, rl_sampler* sampler, HipBuffer<unsigned>* words,
                      uint64_t* n_records, uint64_t* n_paths, rl_render_stats* stats, LightPassSecond* second, Shoot&& shoot) {
    if (per_path)
        return light_pass_paths(ctx, params, nb_primitive, RL_VPL_ALL, kind, sampler, words, n_records, n_paths, stats,
                                [&](bool write, unsigned groups, size_t lds, const RenderConst& rc, const StackConf& stc, const VplPathsConst& pc) {
            shoot(write ? 2 : 1, groups, lds, rc, stc, VplConst{}, pc);
        }, second);
    return light_pass_serial(ctx, params, nb_primitive, RL_VPL_ALL, kind, sampler, words, n_records, n_paths, stats,
                             [&](size_t lds, const RenderConst& rc, const StackConf& stc, const VplConst& vc) { shoot(0, 1u, lds, rc, stc, vc, VplPathsConst{}); }, second);
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
static int beam_generate(bool per_path, rl_context* ctx, const rl_path_params* params, uint32_t nb_primitive, rl_sampler* sampler, rl_beam_set** out, rl_render_stats* stats) {
    int rcode;
    if ((rcode = check_beam_generate(ctx, params, nb_primitive, sampler, out)) != RL_OK) return rcode;
    HIP_OK(hipSetDevice(ctx->device));
    auto set = new_handle<rl_beam_set>(ctx);
    if ((rcode = light_pass(per_path, ctx, params, nb_primitive, kBeamPass, sampler, &set->words, &set->n_beams, &set->n_paths, stats, nullptr,
                            [&](int which, unsigned groups, size_t lds, const RenderConst& rc, const StackConf& stc, const VplConst& vc, const VplPathsConst& pc) {
            (ctx->lds_scene ? launch_beamgen_lds : launch_beamgen_stream)(which, ctx->single_bsdf ? ctx->bsdf_type : -1, dim3(groups), dim3(256), lds, ctx->stream, rc, ctx->ds, stc, vc, pc);
        })) != RL_OK) return rcode;
    *out = set.release();
    return RL_OK;
}
extern "C" int rl_beam_generate(rl_context* ctx, const rl_path_params* params, uint32_t nb_primitive, rl_sampler* sampler, rl_beam_set** out, rl_render_stats* stats) {
    return beam_generate(false, ctx, params, nb_primitive, sampler, out, stats);
}
extern "C" int rl_beam_generate_paths(rl_context* ctx, const rl_path_params* params, uint32_t nb_primitive, rl_sampler* sampler, rl_beam_set** out, rl_render_stats* stats) {
    return beam_generate(true, ctx, params, nb_primitive, sampler, out, stats);
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
extern "C" void rl_beam_destroy(rl_beam_set* set) { destroy_handle(set); }
extern "C" int rl_beam_map_build_words(rl_context* ctx, const uint32_t* words, size_t n_beams, uint64_t n_paths, float radius, rl_beam_map** out) {
    if (!ctx || !out || (n_beams && !words)) return RL_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int rcode;
    if ((rcode = check_beam_scene(ctx)) != RL_OK || (rcode = check_photon_radius(radius)) != RL_OK) return rcode;
    if (n_paths == 0) { rl_set_error("a beam map needs the number of light paths its beams come from (n_paths >= 1)"); return RL_ERR_INVALID_ARGUMENT; }
    auto map = new_handle<rl_beam_map>(ctx);
    BeamHalfHost host;
    if ((rcode = beam_half_build(&map->half, &host, ctx->device, words, n_beams, radius)) != RL_OK) return rcode;
    map->n_beams = n_beams; map->n_paths = n_paths; map->radius = radius;
    *out = map.release();
    return RL_OK;
}
extern "C" int rl_beam_map_build(rl_context* ctx, const rl_beam_set* set, float radius, rl_beam_map** out) {
    if (!ctx || !set || !out) return RL_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int rcode;
    std::vector<uint32_t> words;
    if ((rcode = set_words_to_host(ctx, set->ctx, "beam set", set->words, (size_t)set->n_beams * RL_BEAM_WORDS, &words)) != RL_OK) return rcode;
    return rl_beam_map_build_words(ctx, words.data(), (size_t)set->n_beams, set->n_paths, radius, out);
}
extern "C" int rl_beam_map_info(const rl_beam_map* map, uint64_t* n_beams, uint64_t* n_sub, uint64_t* n_nodes, uint64_t* n_paths, float* radius) {
    if (!map) return RL_ERR_INVALID_ARGUMENT;
    if (n_beams) *n_beams = map->n_beams;
    if (n_sub) *n_sub = map->half.n_sub;
    if (n_nodes) *n_nodes = map->half.n_nodes;
    if (n_paths) *n_paths = map->n_paths;
    if (radius) *radius = map->radius;
    return RL_OK;
}
extern "C" int rl_beam_map_read(const rl_beam_map* map, size_t node_capacity, float* node_boxes, uint32_t* node_links, size_t beam_capacity, float* beams) {
    if (!map || !node_boxes || !node_links || !beams) return RL_ERR_INVALID_ARGUMENT;
    if (node_capacity < map->half.n_nodes || beam_capacity < map->half.n_sub) { rl_set_error("rl_beam_map_read: a capacity is too small"); return RL_ERR_INVALID_ARGUMENT; }
    HIP_OK(hipSetDevice(map->device));
    return beam_half_read(map->half, node_boxes, node_links, beams);
}
extern "C" void rl_beam_map_destroy(rl_beam_map* map) { destroy_handle(map); }
extern "C" int rl_render_beams(rl_context* ctx, const rl_beam_map* map, uint32_t spp, int32_t seed_variant, uint32_t shard_index, uint32_t shard_count,
                               const uint64_t* block_seeds, size_t n_blocks, float* out_rgb, rl_render_stats* stats) {
    if (!map) return RL_ERR_INVALID_ARGUMENT;
    static const GatherKind kind{"photon-beams", "beam map", check_beam_scene, 1, {STAT_BEAM_ACCEPTED}, {STAT_BEAM_ACCEPTED_HI}};      // reserved[1] = beams accepted
    return render_gather(ctx, kind, map->ctx, spp, seed_variant, shard_index, shard_count, block_seeds, n_blocks, out_rgb, stats,
                         [&](bool lds_scene, dim3 grid, size_t lds, hipStream_t st, const RenderConst& rc, const StackConf& stc) {
        (lds_scene ? launch_beam_lds : launch_beam_stream)(grid, dim3(256), lds, st, rc, ctx->ds, stc, beam_half_const(map->half, map->radius, map->n_paths));
    });
}
