// pplane_render.hip.h — the host side of the photon planes (included by wavefront.hip after beam_render.hip.h; host code only): the plane pass (rl_pplane_generate,
// rl_pplane_generate_paths: the light-pass sequences of the beam pass with a second record array, over k_pplane_generate / k_pplane_shoot, pplanegen.hip.h), the
// map of two trees (rl_pplane_map_*: the surface beams into a BeamHalf, beam_render.hip.h, the planes through the plane tree of plane-single, on the host or —
// option pplane_tree_device — by plane_tree_run's kernels) and rl_render_photon_planes, which goes through render_gather with k_pplane_gather (pplane.hip.h).
// IntegratorVolPrimitives with primitives = Planes: src/integrators/explicit/vol_primitives.rs:256-435, 608-790.

struct rl_pplane_set {
    const rl_context* ctx;            // the context that made it (compared, never dereferenced)
    int device;
    HipBuffer<unsigned> planes;       // [n_planes][RL_PLANE_WORDS]
    HipBuffer<unsigned> beams;        // [n_beams][RL_BEAM_WORDS]
    uint64_t n_planes = 0, n_beams = 0, n_paths = 0;
};
struct rl_pplane_map {
    const rl_context* ctx;
    int device;
    BeamHalf half;                    // the surface beams' sub-beams and the beam tree over them
    HipBuffer<float4> plane_nodes;    // [n_plane_nodes][2]
    HipBuffer<float4> planes;         // [n_planes][4], in leaf order
    uint64_t n_beams = 0, n_planes = 0, n_plane_nodes = 0, n_paths = 0;
    float radius = 0.0f;
};
static const LightPassKind kPPlanePass{RL_PLANE_WORDS, "photon-planes: fewer than nb_primitive planes stored within RL_VPL_MAX_PATHS light paths"};
static constexpr unsigned kPPlaneBeamMax = (unsigned)RL_BEAM_MAX + kDepthCap;      // the surface beams a plane pass may store before its last path
static const char* const kPPlaneTooManyBeams =
    "photon-planes: more than RL_BEAM_MAX + 2048 surface beams arose before nb_primitive planes were stored (the medium scatters too seldom for this nb_primitive)";
static int check_pplane_scene(const rl_context* ctx) { return check_medium(ctx, "photon planes"); }
// what both generation entry points refuse before any kernel runs: what check_beam_generate refuses, with its codes, and a depth limit under which no plane exists
static int check_pplane_generate(const rl_context* ctx, const rl_path_params* params, uint32_t nb_primitive, const rl_sampler* sampler, rl_pplane_set** out) {
    if (!ctx || !params || !sampler || !out) return RL_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (nb_primitive == 0 || nb_primitive > (uint32_t)RL_BEAM_MAX) { rl_set_error("nb_primitive must be 1 .. RL_BEAM_MAX"); return RL_ERR_INVALID_ARGUMENT; }
    // a plane needs two edges that leave volume vertices: the light vertex's edge, V1's edge and V2's edge, and V2 is expanded only when 3 < max_depth
    // (pplanegen.hip.h: gnew < max_depth); below that the reference shoots for ever
    if (params->has_max_depth && params->max_depth <= 3) { rl_set_error("photon planes need max_depth >= 4 (no light path holds a plane otherwise, and the reference never stops shooting)"); return RL_ERR_INVALID_ARGUMENT; }
    int rcode;
    if ((rcode = check_vpl_scene(ctx)) != RL_OK || (rcode = check_pplane_scene(ctx)) != RL_OK) return rcode;
    if (ctx->has_directional) { rl_set_error("photon planes do not take a directional light (with a medium the light paths of vpl refuse it)"); return RL_ERR_UNSUPPORTED; }
    return RL_OK;
}
static int pplane_generate(bool per_path, rl_context* ctx, const rl_path_params* params, uint32_t nb_primitive, rl_sampler* sampler, rl_pplane_set** out, rl_render_stats* stats) {
    int rcode;
    if ((rcode = check_pplane_generate(ctx, params, nb_primitive, sampler, out)) != RL_OK) return rcode;
    HIP_OK(hipSetDevice(ctx->device));
    auto set = new_handle<rl_pplane_set>(ctx);
    LightPassSecond second{RL_BEAM_WORDS, kPPlaneBeamMax, kPPlaneTooManyBeams, &set->beams, &set->n_beams};
    if ((rcode = light_pass(per_path, ctx, params, nb_primitive, kPPlanePass, sampler, &set->planes, &set->n_planes, &set->n_paths, stats, &second,
                            [&](int which, unsigned groups, size_t lds, const RenderConst& rc, const StackConf& stc, const VplConst& vc, const VplPathsConst& pc) {
            PPlaneGenConst xc{};
            xc.beam_words = second.d_words; xc.beam_cap = second.cap; xc.beam_max = second.max_records; xc.beam_offsets = second.d_offsets;
            (ctx->lds_scene ? launch_pplanegen_lds : launch_pplanegen_stream)(which, ctx->single_bsdf ? ctx->bsdf_type : -1, dim3(groups), dim3(256), lds, ctx->stream, rc, ctx->ds, stc, vc, pc, xc);
        })) != RL_OK) return rcode;
    *out = set.release();
    return RL_OK;
}
extern "C" int rl_pplane_generate(rl_context* ctx, const rl_path_params* params, uint32_t nb_primitive, rl_sampler* sampler, rl_pplane_set** out, rl_render_stats* stats) {
    return pplane_generate(false, ctx, params, nb_primitive, sampler, out, stats);
}
extern "C" int rl_pplane_generate_paths(rl_context* ctx, const rl_path_params* params, uint32_t nb_primitive, rl_sampler* sampler, rl_pplane_set** out, rl_render_stats* stats) {
    return pplane_generate(true, ctx, params, nb_primitive, sampler, out, stats);
}
extern "C" int rl_pplane_info(const rl_pplane_set* set, uint64_t* n_planes, uint64_t* n_beams, uint64_t* n_paths) {
    if (!set) return RL_ERR_INVALID_ARGUMENT;
    if (n_planes) *n_planes = set->n_planes;
    if (n_beams) *n_beams = set->n_beams;
    if (n_paths) *n_paths = set->n_paths;
    return RL_OK;
}
extern "C" int rl_pplane_read(const rl_pplane_set* set, uint32_t* plane_words, size_t n_plane_words, uint32_t* beam_words, size_t n_beam_words) {
    if (!set || !plane_words || !beam_words || n_plane_words != set->n_planes * RL_PLANE_WORDS || n_beam_words != set->n_beams * RL_BEAM_WORDS) return RL_ERR_INVALID_ARGUMENT;
    HIP_OK(hipSetDevice(set->device));
    HIP_OK(hipMemcpy(plane_words, set->planes.get(), n_plane_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(beam_words, set->beams.get(), n_beam_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RL_OK;
}
extern "C" void rl_pplane_destroy(rl_pplane_set* set) { destroy_handle(set); }
// both trees.  The beams are host records.  The planes are host records (plane_words), or records on the device (d_plane_words, plane_words NULL) when the
// device build is to read a set in place.  Words 16 and 17 of a plane record are 0: a caller's record that sets them is refused, so that the type word the
// device build packs beside d1 is the 0 the host build packs and both builds give the same bytes.
static int pplane_map_build(rl_context* ctx, const uint32_t* beam_words, size_t n_beams, const uint32_t* plane_words, size_t n_planes, const unsigned* d_plane_words,
                            uint64_t n_paths, float radius, rl_pplane_map** out) {
    int rcode;
    if ((rcode = check_pplane_scene(ctx)) != RL_OK || (rcode = check_photon_radius(radius)) != RL_OK) return rcode;
    if (n_paths == 0) { rl_set_error("a photon-plane map needs the number of light paths its records come from (n_paths >= 1)"); return RL_ERR_INVALID_ARGUMENT; }
    if (n_planes > kElementTreeMax) { rl_set_error("too many planes"); return RL_ERR_INVALID_ARGUMENT; }
    if (plane_words)
        for (size_t i = 0; i < n_planes; i++)
            if (plane_words[i * RL_PLANE_WORDS + 16] | plane_words[i * RL_PLANE_WORDS + 17]) { rl_set_error("words 16 and 17 of a photon-plane record must be 0"); return RL_ERR_INVALID_ARGUMENT; }
    // ---- the surface beams: split and beam tree
    auto map = new_handle<rl_pplane_map>(ctx);
    BeamHalfHost host;                                      // lives until the plane half is built too
    if ((rcode = beam_half_build(&map->half, &host, ctx->device, beam_words, n_beams, radius)) != RL_OK) return rcode;
    // ---- the planes: plane-single's tree over the same geometry layout
    size_t n_plane_nodes = 0;
    if (knob_on(ctx, K_PPLANE_TREE_DEVICE) && n_planes > 0) {
        const unsigned n = (unsigned)n_planes;
        n_plane_nodes = photon_tree_node_count(n);
        HipBuffer<unsigned> uploaded;
        if (!d_plane_words) {
            if ((rcode = uploaded.ensure(n_planes * RL_PLANE_WORDS)) != RL_OK) return rcode;
            HIP_OK(hipMemcpyAsync(uploaded.get(), plane_words, n_planes * RL_PLANE_WORDS * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
            d_plane_words = uploaded.get();
        }
        if ((rcode = map->plane_nodes.ensure(2 * n_plane_nodes)) != RL_OK || (rcode = map->planes.ensure(4 * n_planes)) != RL_OK) return rcode;
        const PlaneTreeJob job{d_plane_words, n, plane_tree_group(ctx), map->plane_nodes.get(), nullptr, map->planes.get()};
        if ((rcode = plane_tree_run(job, ctx->stream, false, nullptr)) != RL_OK) return rcode;      // returns synchronised: `uploaded` may go
    } else {
        ElementTree plane_tree;
        if ((rcode = build_plane_tree(plane_words, n_planes, &plane_tree)) != RL_OK) return rcode;
        n_plane_nodes = plane_tree.n_nodes();
        const std::vector<float4> h_nodes = pack_tree_nodes(plane_tree);
        std::vector<float4> h_planes(4 * n_planes);
        for (size_t i = 0; i < n_planes; i++) {
            float f[14];
            std::memcpy(f, &plane_words[(size_t)plane_tree.order[i] * RL_PLANE_WORDS], sizeof f);      // o, d0, d1, length0, length1, radiance
            h_planes[4 * i] = make_float4(f[0], f[1], f[2], f[9]);
            h_planes[4 * i + 1] = make_float4(f[3], f[4], f[5], f[10]);
            h_planes[4 * i + 2] = make_float4(f[6], f[7], f[8], 0.0f);
            h_planes[4 * i + 3] = make_float4(f[11], f[12], f[13], 0.0f);
        }
        if ((rcode = upload_tree(h_nodes, h_planes, &map->plane_nodes, &map->planes)) != RL_OK) return rcode;
    }
    map->n_beams = n_beams; map->n_planes = n_planes; map->n_plane_nodes = n_plane_nodes; map->n_paths = n_paths; map->radius = radius;
    *out = map.release();
    return RL_OK;
}
extern "C" int rl_pplane_map_build_words(rl_context* ctx, const uint32_t* beam_words, size_t n_beams, const uint32_t* plane_words, size_t n_planes, uint64_t n_paths,
                                         float radius, rl_pplane_map** out) {
    if (!ctx || !out || (n_beams && !beam_words) || (n_planes && !plane_words)) return RL_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    return pplane_map_build(ctx, beam_words, n_beams, plane_words, n_planes, nullptr, n_paths, radius, out);
}
extern "C" int rl_pplane_map_build(rl_context* ctx, const rl_pplane_set* set, float radius, rl_pplane_map** out) {
    if (!ctx || !set || !out) return RL_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int rcode;
    std::vector<uint32_t> beams, planes;
    if ((rcode = set_words_to_host(ctx, set->ctx, "photon-plane set", set->beams, (size_t)set->n_beams * RL_BEAM_WORDS, &beams)) != RL_OK) return rcode;
    const bool in_place = knob_on(ctx, K_PPLANE_TREE_DEVICE) && set->n_planes > 0;      // the device build reads the set's planes where they are
    if (!in_place && (rcode = set_words_to_host(ctx, set->ctx, "photon-plane set", set->planes, (size_t)set->n_planes * RL_PLANE_WORDS, &planes)) != RL_OK) return rcode;
    return pplane_map_build(ctx, beams.data(), (size_t)set->n_beams, in_place ? nullptr : planes.data(), (size_t)set->n_planes, in_place ? set->planes.get() : nullptr, set->n_paths,
                            radius, out);
}
extern "C" int rl_pplane_map_info(const rl_pplane_map* map, uint64_t* n_beams, uint64_t* n_sub, uint64_t* n_beam_nodes, uint64_t* n_planes, uint64_t* n_plane_nodes,
                                  uint64_t* n_paths, float* radius) {
    if (!map) return RL_ERR_INVALID_ARGUMENT;
    if (n_beams) *n_beams = map->n_beams;
    if (n_sub) *n_sub = map->half.n_sub;
    if (n_beam_nodes) *n_beam_nodes = map->half.n_nodes;
    if (n_planes) *n_planes = map->n_planes;
    if (n_plane_nodes) *n_plane_nodes = map->n_plane_nodes;
    if (n_paths) *n_paths = map->n_paths;
    if (radius) *radius = map->radius;
    return RL_OK;
}
// which: 0 = the beam tree and the sub-beams ([n_sub][12] f32), 1 = the plane tree and the planes ([n_planes][16] f32)
extern "C" int rl_pplane_map_read(const rl_pplane_map* map, int which, size_t node_capacity, float* node_boxes, uint32_t* node_links, size_t element_capacity, float* elements) {
    if (!map || !node_boxes || !node_links || !elements || which < 0 || which > 1) return RL_ERR_INVALID_ARGUMENT;
    const size_t n_nodes = (size_t)(which ? map->n_plane_nodes : map->half.n_nodes), n_elements = (size_t)(which ? map->n_planes : map->half.n_sub);
    if (node_capacity < n_nodes || element_capacity < n_elements) { rl_set_error("rl_pplane_map_read: a capacity is too small"); return RL_ERR_INVALID_ARGUMENT; }
    HIP_OK(hipSetDevice(map->device));
    if (which) return read_tree(map->plane_nodes, n_nodes, map->planes, n_elements * 4, node_boxes, node_links, elements);
    return beam_half_read(map->half, node_boxes, node_links, elements);
}
extern "C" void rl_pplane_map_destroy(rl_pplane_map* map) { destroy_handle(map); }
extern "C" int rl_render_photon_planes(rl_context* ctx, const rl_pplane_map* map, uint32_t spp, int32_t seed_variant, uint32_t shard_index, uint32_t shard_count,
                                       const uint64_t* block_seeds, size_t n_blocks, float* out_rgb, rl_render_stats* stats) {
    if (!map) return RL_ERR_INVALID_ARGUMENT;
    // reserved[1] = beams accepted, [2] = planes intersected, [3] = of those visible; the counters take every statistics row, so the samples are derived
    static const GatherKind kind{"photon-planes", "photon-plane map", check_pplane_scene, 3, {STAT_PPLANE_BEAMS, STAT_PPLANE_ISECT, STAT_PPLANE_VISIBLE},
                                 {STAT_PPLANE_BEAMS_HI, STAT_PPLANE_ISECT_HI, STAT_PPLANE_VISIBLE_HI}, 2, true};
    const int rcode = render_gather(ctx, kind, map->ctx, spp, seed_variant, shard_index, shard_count, block_seeds, n_blocks, out_rgb, stats,
                                    [&](bool lds_scene, dim3 grid, size_t lds, hipStream_t st, const RenderConst& rc, const StackConf& stc) {
        PPlaneConst pc{};
        pc.beam = beam_half_const(map->half, map->radius, map->n_paths);
        pc.nodes = map->plane_nodes.get(); pc.planes = map->planes.get(); pc.n_nodes = (unsigned)map->n_plane_nodes;
        (lds_scene ? launch_pplane_lds : launch_pplane_stream)(grid, dim3(256), lds, st, rc, ctx->ds, stc, pc);
    });
    if (rcode == RL_OK && stats) stats->shadow_rays = stats->reserved[2];      // each plane the ray meets takes one visibility ray
    return rcode;
}
