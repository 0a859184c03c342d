// gather_render.hip.h — the host side of the two integrators that gather along camera beams (included by wavefront.hip after rl_context, RenderFrame and the
// launch helpers; host code only): the beam radiance estimate (rl_photon_map_*, rl_photon_tree_build_device, rl_render_bre) and the single-scattering photon
// planes (rl_plane_*, rl_plane_map_*, rl_render_plane_single).  Both upload an element tree (host/photontree.h) in the gather's node format and render through
// render_gather: one launch of beam_gather (gather.hip.h) over this shard's blocks.  The uncorrelated photon planes (rl_render_plane_uncorrelated) have no tree
// and a kernel of their own (uplane.hip.h), and go through render_gather for everything else.

// an element tree -> its nodes in the gather's format (launch.h: BreConst::nodes)
static std::vector<float4> pack_tree_nodes(const ElementTree& tree) {
    std::vector<float4> h_nodes(2 * tree.n_nodes());
    for (size_t i = 0; i < tree.n_nodes(); i++) {
        const float* b = &tree.boxes[6 * i];
        const uint32_t skip = tree.links[3 * i], fc = tree.links[3 * i + 1] << 3 | tree.links[3 * i + 2];
        float fs, ff;
        std::memcpy(&fs, &skip, sizeof fs); std::memcpy(&ff, &fc, sizeof ff);
        h_nodes[2 * i] = make_float4(b[0], b[1], b[2], b[3]);
        h_nodes[2 * i + 1] = make_float4(b[4], b[5], fs, ff);
    }
    return h_nodes;
}
// and back: nodes in the gather's format -> the arrays rl_photon_tree_build writes
static void unpack_tree_nodes(const std::vector<float4>& h_nodes, size_t n_nodes, float* node_boxes, uint32_t* node_links) {
    for (size_t i = 0; i < n_nodes; i++) {
        const float4 a = h_nodes[2 * i], b = h_nodes[2 * i + 1];
        const float box[6] = {a.x, a.y, a.z, a.w, b.x, b.y};
        std::memcpy(node_boxes + 6 * i, box, sizeof box);
        uint32_t skip, fc;
        std::memcpy(&skip, &b.z, sizeof skip); std::memcpy(&fc, &b.w, sizeof fc);
        node_links[3 * i] = skip; node_links[3 * i + 1] = fc >> 3; node_links[3 * i + 2] = fc & 7u;
    }
}
// a tree's nodes and its elements in leaf order, to the current device ...
static int upload_tree(const std::vector<float4>& h_nodes, const std::vector<float4>& h_elements, HipBuffer<float4>* nodes, HipBuffer<float4>* elements) {
    int rcode;
    if ((rcode = nodes->ensure(h_nodes.size())) != RL_OK || (rcode = elements->ensure(h_elements.size())) != RL_OK) return rcode;
    HIP_OK(hipMemcpy(nodes->get(), h_nodes.data(), h_nodes.size() * sizeof(float4), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(elements->get(), h_elements.data(), h_elements.size() * sizeof(float4), hipMemcpyHostToDevice));
    return RL_OK;
}
// ... and back from it: the nodes unpacked, the n_quads float4 of the elements as they are
static int read_tree(const HipBuffer<float4>& nodes, size_t n_nodes, const HipBuffer<float4>& elements, size_t n_quads, float* node_boxes, uint32_t* node_links, float* out) {
    std::vector<float4> h_nodes(2 * n_nodes);
    HIP_OK(hipMemcpy(h_nodes.data(), nodes.get(), h_nodes.size() * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(out, elements.get(), n_quads * sizeof(float4), hipMemcpyDeviceToHost));
    unpack_tree_nodes(h_nodes, n_nodes, node_boxes, node_links);
    return RL_OK;
}
// what every rl_*_destroy of a set or a map on a device does
template <class T>
static void destroy_handle(T* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;
}

// What the two gathers do not share beyond their constants and their launch
struct GatherKind {
    const char* who;                            // the integrator's name in the messages
    const char* map;                            // and its map's
    int (*check_scene)(const rl_context*);
    int n_counters;                             // the leaf's walk counters (gather.hip.h) ...
    int lo[3], hi[3];                           // ... and the statistics rows of their low and high parts
    uint64_t draws = 2;                         // draws per camera sample: the 256 lanes of a block enter its stream with 32-bit jumps
    bool derive_samples = false;                // the kernel's counters take every statistics row: camera_samples = owned pixels * spp, which is what the lanes count
};
// rl_render_bre / rl_render_plane_single: the argument checks, the frame, one launch — launch(lds_scene, grid, lds_bytes, stream, rc, stc) — between two events,
// the finish.  stats: reserved[0] = nodes entered, reserved[1 + k] = the leaf's counter k; extension rays and draws follow from the samples (one ray, 2 draws each)
template <class Launch>
static int render_gather(rl_context* ctx, const GatherKind& kind, const rl_context* map_ctx, uint32_t spp, int32_t seed_variant, uint32_t shard_index, uint32_t shard_count,
                         const uint64_t* block_seeds, size_t n_blocks, float* out_rgb, rl_render_stats* stats, Launch&& launch) {
    int rcode;
    if ((rcode = check_frame(ctx, spp, block_seeds, n_blocks, out_rgb)) != RL_OK) return rcode;
    if ((rcode = kind.check_scene(ctx)) != RL_OK) return rcode;
    if (map_ctx != ctx) { rl_set_error(std::string("the ") + kind.map + " belongs to another context"); return RL_ERR_INVALID_ARGUMENT; }
    if (shard_index >= (shard_count ? shard_count : 1)) return RL_ERR_INVALID_ARGUMENT;
    if (spp > (uint32_t)RL_VPL_MAX_SPP) { rl_set_error(std::string(kind.who) + " takes at most RL_VPL_MAX_SPP spp (a block's stream is entered with 32-bit jumps, 2 draws per sample)"); return RL_ERR_UNSUPPORTED; }
    if (256ull * spp * kind.draws > 0xffffffffull) { rl_set_error(std::string(kind.who) + ": 256 * spp * (draws per sample) exceeds 2^32 - 1, the reach of the jumps a block's stream is entered with"); return RL_ERR_UNSUPPORTED; }
    HIP_OK(hipSetDevice(ctx->device));
    RenderFrame fr(ctx, block_seeds, n_blocks, out_rgb, 0, nullptr, stats, shard_index, shard_count);
    const unsigned n_owned = (unsigned)fr.owned.size();
    if ((rcode = fr.alloc_tables()) != RL_OK || (rcode = fr.alloc_output(std::max(n_owned, 1u))) != RL_OK) return rcode;
    if ((rcode = fr.upload(false, true)) != RL_OK || (rcode = fr.zero_rows()) != RL_OK) return rcode;
    RenderConst rc = fr.render_const(spp, RL_STREAM_REFERENCE_ORDER, seed_variant);
    rc.n_items = fr.n_pixels;
    StackConf stc;
    if ((rcode = stack_conf(ctx, std::max(n_owned, 1u) * 256u, &stc)) != RL_OK) return rcode;
    const size_t lds = traversal_lds_bytes(ctx, ctx->lds_scene, 256, false);
    const hipStream_t st = fr.st;
    if ((rcode = fr.grow_events(2)) != RL_OK) return rcode;
    if (fr.timing) hipEventRecord(ctx->events[0], st);
    if (n_owned > 0) launch(ctx->lds_scene, dim3(n_owned), lds, st, rc, stc);
    if (fr.timing) hipEventRecord(ctx->events[1], st);
    if ((rcode = fr.download()) != RL_OK) return rcode;
    if (stats) {
        // (the rows of vertices / extension_rays / shadow_rays carried the high parts of the walk counters)
        if (kind.derive_samples) stats->camera_samples = (uint64_t)fr.n_pixels * spp;
        stats->reserved[0] = gather_merge24(fr.totals, STAT_GATHER_NODES, STAT_GATHER_NODES_HI);
        for (int k = 0; k < kind.n_counters; k++) stats->reserved[1 + k] = gather_merge24(fr.totals, kind.lo[k], kind.hi[k]);
        stats->vertices = 0; stats->extension_rays = stats->camera_samples; stats->shadow_rays = 0; stats->rng_draws = 2 * stats->camera_samples;
        stats->iterations = 1; stats->kernel_launches = n_owned > 0 ? 1 : 0;
        if (fr.timing) {
            float t = 0.0f;
            if (hipEventElapsedTime(&t, ctx->events[0], ctx->events[1]) == hipSuccess) stats->ms_other = t;
            (void)hipGetLastError();
        }
    }
    return RL_OK;
}

// ---- IntegratorVolPrimitives' beam radiance estimate (vol_primitives.rs:568-805): the photons are the records of an rl_vpl_generate(RL_VPL_VOLUME) set
// (convert_photons stores what convert_vpl stores under `-v volume`, from the same light paths, and stops on the same count); rl_photon_map_build sorts them into
// the photon tree on the host (host/photontree.cpp) and uploads tree and photons, rl_render_bre gathers them along every camera ray (k_bre_gather, bre.hip.h)
struct rl_photon_map {
    const rl_context* ctx;            // the context that made it (compared, never dereferenced)
    int device;
    HipBuffer<float4> nodes;          // [n_nodes][2]
    HipBuffer<float4> photons;        // [n_photons][3], in leaf order
    uint64_t n_photons = 0, n_nodes = 0, n_paths = 0;
    float radius = 0.0f;
};
static int check_bre_scene(const rl_context* ctx) {
    if (ctx->ds.medium.enabled == 0) { rl_set_error("the beam radiance estimate needs a medium (add -m; the reference panics, vol_primitives.rs:575)"); return RL_ERR_UNSUPPORTED; }
    return RL_OK;
}
extern "C" int rl_photon_map_build(rl_context* ctx, const rl_vpl_set* set, float radius, rl_photon_map** out) {
    if (!ctx || !set || !out) return RL_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int rcode;
    if ((rcode = check_bre_scene(ctx)) != RL_OK) return rcode;
    if (set->ctx != ctx) { rl_set_error("the VPL set belongs to another context"); return RL_ERR_INVALID_ARGUMENT; }
    if ((rcode = check_photon_radius(radius)) != RL_OK) return rcode;
    HIP_OK(hipSetDevice(ctx->device));
    std::vector<uint32_t> words((size_t)set->n_vpl * RL_VPL_WORDS);
    HIP_OK(hipMemcpy(words.data(), set->words.get(), words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < set->n_vpl; i++)
        if (words[i * RL_VPL_WORDS] != (uint32_t)RL_VPL_KIND_VOLUME) { rl_set_error("a photon map takes volume records only: generate the set with RL_VPL_VOLUME"); return RL_ERR_INVALID_ARGUMENT; }
    ElementTree tree;
    if ((rcode = build_photon_tree(words.data(), set->n_vpl, radius, &tree)) != RL_OK) return rcode;
    const size_t n_nodes = tree.n_nodes();
    const std::vector<float4> h_nodes = pack_tree_nodes(tree);
    std::vector<float4> h_photons(3 * (size_t)set->n_vpl);
    for (size_t i = 0; i < set->n_vpl; i++) {
        float f[9];
        std::memcpy(f, &words[(size_t)tree.order[i] * RL_VPL_WORDS + 4], sizeof f);     // pos, radiance, d_in
        h_photons[3 * i] = make_float4(f[0], f[1], f[2], 0.0f);
        h_photons[3 * i + 1] = make_float4(f[3], f[4], f[5], 0.0f);
        h_photons[3 * i + 2] = make_float4(f[6], f[7], f[8], 0.0f);
    }
    auto map = std::make_unique<rl_photon_map>();
    map->ctx = ctx; map->device = ctx->device;
    if ((rcode = upload_tree(h_nodes, h_photons, &map->nodes, &map->photons)) != RL_OK) return rcode;
    map->n_photons = set->n_vpl; map->n_nodes = n_nodes; map->n_paths = set->n_paths; map->radius = radius;
    *out = map.release();
    return RL_OK;
}
// The device build (kernels/phototree.hip.h): the same map from kernels alone.  photon_tree_run's check pass stands for the host's loops over downloaded words.
static unsigned photon_tree_group(const rl_context* ctx) {
    if (!ctx->knobs.has(K_PHOTON_TREE_GROUP_PHOTONS)) return (unsigned)RL_PHOTON_TREE_GROUP_PHOTONS;
    return (unsigned)std::min<long long>(std::max<long long>(4, ctx->knobs.i(K_PHOTON_TREE_GROUP_PHOTONS, 0)), RL_PHOTON_TREE_GROUP_PHOTONS);
}
extern "C" int rl_photon_map_build_device(rl_context* ctx, const rl_vpl_set* set, float radius, rl_photon_map** out, float* ms_kernels) {
    if (!ctx || !set || !out) return RL_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (ms_kernels) *ms_kernels = 0.0f;
    int rcode;
    if ((rcode = check_bre_scene(ctx)) != RL_OK) return rcode;
    if (set->ctx != ctx) { rl_set_error("the VPL set belongs to another context"); return RL_ERR_INVALID_ARGUMENT; }
    if ((rcode = check_photon_radius(radius)) != RL_OK) return rcode;
    if (set->n_vpl > kElementTreeMax) { rl_set_error("too many photons"); return RL_ERR_INVALID_ARGUMENT; }
    HIP_OK(hipSetDevice(ctx->device));
    const unsigned n = (unsigned)set->n_vpl, n_nodes = photon_tree_node_count(n);
    auto map = std::make_unique<rl_photon_map>();
    map->ctx = ctx; map->device = ctx->device;
    if ((rcode = map->nodes.ensure(2 * (size_t)n_nodes)) != RL_OK || (rcode = map->photons.ensure(3 * (size_t)n)) != RL_OK) return rcode;
    const PhotonTreeJob job{set->words.get(), n, radius, photon_tree_group(ctx), true, map->nodes.get(), nullptr, map->photons.get()};
    if ((rcode = photon_tree_run(job, ctx->stream, !ctx->knobs.has(K_NO_EVENTS), ms_kernels)) != RL_OK) return rcode;
    map->n_photons = n; map->n_nodes = n_nodes; map->n_paths = set->n_paths; map->radius = radius;
    *out = map.release();
    return RL_OK;
}
extern "C" int rl_photon_tree_build_device(rl_context* ctx, const uint32_t* words, size_t n_photons, float radius, size_t node_capacity, size_t* n_nodes,
                                           float* node_boxes, uint32_t* node_links, uint32_t* order) {
    if (!ctx || !n_nodes || (n_photons && !words)) return RL_ERR_INVALID_ARGUMENT;
    int rcode;
    if ((rcode = check_photon_radius(radius)) != RL_OK) return rcode;
    if (n_photons > kElementTreeMax) { rl_set_error("too many photons"); return RL_ERR_INVALID_ARGUMENT; }      // before any allocation
    const bool size_only = !node_boxes && !node_links && !order;
    if (!size_only && (!node_boxes || !node_links || !order)) return RL_ERR_INVALID_ARGUMENT;
    if (n_photons == 0) { *n_nodes = 0; return RL_OK; }
    HIP_OK(hipSetDevice(ctx->device));
    const unsigned n = (unsigned)n_photons, count = photon_tree_node_count(n);
    HipBuffer<unsigned> d_words, d_order;
    HipBuffer<float4> d_nodes;
    if ((rcode = d_words.ensure(n_photons * RL_VPL_WORDS)) != RL_OK) return rcode;
    HIP_OK(hipMemcpyAsync(d_words.get(), words, n_photons * RL_VPL_WORDS * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    if (size_only || node_capacity < count) {
        // the host build refuses a bad record before it looks at the capacity: the check pass alone
        const PhotonTreeJob check{d_words.get(), n, radius, photon_tree_group(ctx), false, nullptr, nullptr, nullptr};
        if ((rcode = photon_tree_run(check, ctx->stream, false, nullptr)) != RL_OK) return rcode;
        HIP_OK(hipStreamSynchronize(ctx->stream));
        *n_nodes = count;
        if (size_only) return RL_OK;
        rl_set_error("rl_photon_tree_build_device: node_capacity is too small");
        return RL_ERR_INVALID_ARGUMENT;
    }
    if ((rcode = d_order.ensure(n)) != RL_OK || (rcode = d_nodes.ensure(2 * (size_t)count)) != RL_OK) return rcode;
    const PhotonTreeJob job{d_words.get(), n, radius, photon_tree_group(ctx), false, d_nodes.get(), d_order.get(), nullptr};
    if ((rcode = photon_tree_run(job, ctx->stream, false, nullptr)) != RL_OK) return rcode;
    HIP_OK(hipStreamSynchronize(ctx->stream));
    *n_nodes = count;
    std::vector<float4> h_nodes(2 * (size_t)count);
    HIP_OK(hipMemcpy(h_nodes.data(), d_nodes.get(), h_nodes.size() * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(order, d_order.get(), (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    unpack_tree_nodes(h_nodes, count, node_boxes, node_links);
    return RL_OK;
}
extern "C" int rl_photon_map_read(const rl_photon_map* map, size_t node_capacity, float* node_boxes, uint32_t* node_links, size_t photon_capacity, float* photons) {
    if (!map || !node_boxes || !node_links || !photons) return RL_ERR_INVALID_ARGUMENT;
    if (node_capacity < map->n_nodes || photon_capacity < map->n_photons) { rl_set_error("rl_photon_map_read: a capacity is too small"); return RL_ERR_INVALID_ARGUMENT; }
    HIP_OK(hipSetDevice(map->device));
    std::vector<float4> h_nodes(2 * (size_t)map->n_nodes), h_photons(3 * (size_t)map->n_photons);
    HIP_OK(hipMemcpy(h_nodes.data(), map->nodes.get(), h_nodes.size() * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(h_photons.data(), map->photons.get(), h_photons.size() * sizeof(float4), hipMemcpyDeviceToHost));
    unpack_tree_nodes(h_nodes, (size_t)map->n_nodes, node_boxes, node_links);
    for (size_t i = 0; i < (size_t)map->n_photons; i++)
        for (int q = 0; q < 3; q++) {
            const float4 v = h_photons[3 * i + q];
            photons[9 * i + 3 * q] = v.x; photons[9 * i + 3 * q + 1] = v.y; photons[9 * i + 3 * q + 2] = v.z;
        }
    return RL_OK;
}
extern "C" int rl_photon_map_info(const rl_photon_map* map, uint64_t* n_photons, uint64_t* n_nodes, uint64_t* n_paths, float* radius) {
    if (!map) return RL_ERR_INVALID_ARGUMENT;
    if (n_photons) *n_photons = map->n_photons;
    if (n_nodes) *n_nodes = map->n_nodes;
    if (n_paths) *n_paths = map->n_paths;
    if (radius) *radius = map->radius;
    return RL_OK;
}
extern "C" void rl_photon_map_destroy(rl_photon_map* map) { destroy_handle(map); }
extern "C" int rl_render_bre(rl_context* ctx, const rl_photon_map* map, uint32_t spp, int32_t seed_variant, uint32_t shard_index, uint32_t shard_count,
                             const uint64_t* block_seeds, size_t n_blocks, float* out_rgb, rl_render_stats* stats) {
    if (!map) return RL_ERR_INVALID_ARGUMENT;
    static const GatherKind kind{"bre", "photon map", check_bre_scene, 1, {STAT_BRE_PHOTONS}, {STAT_BRE_PHOTONS_HI}};      // reserved[1] = photons gathered
    return render_gather(ctx, kind, map->ctx, spp, seed_variant, shard_index, shard_count, block_seeds, n_blocks, out_rgb, stats,
                         [&](bool lds_scene, dim3 grid, size_t lds, hipStream_t st, const RenderConst& rc, const StackConf& stc) {
        BreConst bc{};
        bc.nodes = map->nodes.get(); bc.photons = map->photons.get(); bc.n_nodes = (unsigned)map->n_nodes;
        bc.radius2 = map->radius * map->radius;                                 // self.radius * self.radius
        bc.kernel = 1.0f / (3.14159265358979323846f * (map->radius * map->radius));       // 1.0 / (PI * self.radius.powi(2))
        bc.norm_photon = 1.0f / (float)map->n_paths;                            // 1.0 / nb_path_shot as f32 (vol_primitives.rs:707)
        (lds_scene ? launch_bre_lds : launch_bre_stream)(ctx->ds.medium.phase != 0, grid, dim3(256), lds, st, rc, ctx->ds, stc, bc);
    });
}

// ---- IntegratorSinglePlane (plane_single.rs): rl_plane_generate makes the planes on one lane (k_plane_generate, plane_generate.hip) and brings them to the
// host, rl_plane_map_build sorts them into the plane tree there (host/planetree.cpp) and uploads tree, planes and lights, rl_render_plane_single gathers them
// along every camera ray (k_plane_gather, plane.hip.h).  The device forms give the same bytes: rl_plane_generate_lanes (k_plane_generate_lanes, one lane per
// iteration) leaves the records on the device, rl_plane_map_build_device builds the tree there (kernels/planetree.hip).
struct rl_plane_set {
    const rl_context* ctx;            // the context that made it (compared, never dereferenced)
    int device = 0;
    // [n_planes][RL_PLANE_WORDS]: on the host (rl_plane_generate), or on the device (rl_plane_generate_lanes) and on the host once something has asked for them
    mutable std::vector<uint32_t> words;
    HipBuffer<unsigned> d_words;
    bool on_device = false;
    uint64_t n_planes = 0, n_gen = 0;
    int strategy = 0;
    int host_words() const {
        if (!on_device || !words.empty() || n_planes == 0) return RL_OK;
        HIP_OK(hipSetDevice(device));
        std::vector<uint32_t> w((size_t)n_planes * RL_PLANE_WORDS);
        HIP_OK(hipMemcpy(w.data(), d_words.get(), w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        words.swap(w);
        return RL_OK;
    }
};
struct rl_plane_map {
    const rl_context* ctx;
    int device;
    HipBuffer<float4> nodes;          // [n_nodes][2]
    HipBuffer<float4> planes;         // [n_planes][4], in leaf order
    HipBuffer<PlaneLight> lights;
    uint64_t n_planes = 0, n_nodes = 0, n_gen = 0, n_lights = 0;
    int strategy = 0;
};
static int plane_generate_serial(rl_context* ctx, uint32_t nb_primitive, int strategy, rl_sampler* sampler, rl_plane_set** out, rl_render_stats* stats);
// what every plane entry point refuses before any kernel runs
static int check_plane_scene(const rl_context* ctx) {
    if (ctx->ds.medium.enabled == 0) { rl_set_error("plane-single needs a medium (add -m; the reference panics, plane_single.rs:303)"); return RL_ERR_UNSUPPORTED; }
    if (ctx->rect_lights_rc != RL_OK) { rl_set_error(ctx->rect_lights_err); return ctx->rect_lights_rc; }
    return RL_OK;
}
static std::vector<PlaneLight> plane_lights(const rl_context* ctx) {
    std::vector<PlaneLight> out;
    for (const RectLight& r : ctx->rect_lights) {
        PlaneLight l{};
        for (int k = 0; k < 3; k++) { l.o[k] = r.o[k]; l.u[k] = r.u[k]; l.v[k] = r.v[k]; l.n[k] = r.n[k]; l.emission[k] = r.emission[k]; }
        l.u_l = r.u_l; l.v_l = r.v_l;
        out.push_back(l);
    }
    return out;
}
static bool knob_on(const rl_context* ctx, int k) { return ctx->knobs.i(k, 0) != 0; }
extern "C" int rl_plane_generate(rl_context* ctx, uint32_t nb_primitive, int strategy, rl_sampler* sampler, rl_plane_set** out, rl_render_stats* stats) {
    if (ctx && knob_on(ctx, K_PLANE_GENERATE_LANES)) return rl_plane_generate_lanes(ctx, nb_primitive, strategy, sampler, out, stats);
    return plane_generate_serial(ctx, nb_primitive, strategy, sampler, out, stats);
}
static int plane_generate_serial(rl_context* ctx, uint32_t nb_primitive, int strategy, rl_sampler* sampler, rl_plane_set** out, rl_render_stats* stats) {
    if (!ctx || !sampler || !out) return RL_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (strategy < RL_PLANE_STRATEGY_UV || strategy > RL_PLANE_STRATEGY_CMIS) { rl_set_error("strategy must be one of RL_PLANE_STRATEGY_*"); return RL_ERR_INVALID_ARGUMENT; }
    if (nb_primitive == 0 || nb_primitive > (uint32_t)RL_VPL_MAX) { rl_set_error("nb_primitive must be 1 .. RL_VPL_MAX"); return RL_ERR_INVALID_ARGUMENT; }
    int rcode;
    if ((rcode = check_plane_scene(ctx)) != RL_OK) return rcode;
    HIP_OK(hipSetDevice(ctx->device));
    const std::vector<PlaneLight> lights = plane_lights(ctx);
    const unsigned cap = nb_primitive + 2u;              // Average / DiscreteMIS store three planes per iteration
    HipBuffer<unsigned> d_words;
    HipBuffer<PlaneLight> d_lights;
    if ((rcode = d_words.ensure((size_t)cap * RL_PLANE_WORDS)) != RL_OK || (rcode = d_lights.ensure(lights.size())) != RL_OK) return rcode;
    const hipStream_t st = ctx->stream;
    HIP_OK(hipMemcpyAsync(d_lights.get(), lights.data(), lights.size() * sizeof(PlaneLight), hipMemcpyHostToDevice, st));
    PlaneGenConst gc{};
    gc.nb_primitive = nb_primitive; gc.cap = cap; gc.strategy = strategy;
    gc.n_lights = (unsigned)lights.size(); gc.lights = d_lights.get();
    for (int k = 0; k < 3; k++) { gc.sigma_t[k] = ctx->ds.medium.sigma_t[k]; gc.sigma_s[k] = ctx->ds.medium.sigma_s[k]; }
    gc.words = d_words.get();
    LaneRun run;
    if ((rcode = run_one_lane(st, stats != nullptr && !ctx->knobs.has(K_NO_EVENTS), sampler, PLANE_GEN_WORDS, &run, [&](unsigned long long* d_gen) {
            gc.gen_state = d_gen; gc.gen_out = d_gen + 4;
            launch_plane_generate(st, gc);
        })) != RL_OK) return rcode;
    const unsigned long long* g = run.words.data() + 4;
    if (g[PLANE_GEN_PLANES] < nb_primitive || g[PLANE_GEN_PLANES] > cap) { rl_set_error("plane-single: the generation stored an unexpected number of planes"); return RL_ERR_HIP; }
    auto set = std::make_unique<rl_plane_set>();
    set->ctx = ctx; set->device = ctx->device;
    set->n_planes = g[PLANE_GEN_PLANES]; set->n_gen = g[PLANE_GEN_ITERATIONS]; set->strategy = strategy;
    set->words.resize((size_t)set->n_planes * RL_PLANE_WORDS);
    HIP_OK(hipMemcpy(set->words.data(), d_words.get(), set->words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if ((rcode = check_plane_records(set->words.data(), (size_t)set->n_planes)) != RL_OK) return rcode;
    for (int i = 0; i < 4; i++) sampler->s[i] = run.words[i];
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->camera_samples = set->n_gen; stats->vertices = set->n_planes; stats->rng_draws = g[PLANE_GEN_DRAWS];
        stats->iterations = 1; stats->kernel_launches = 1; stats->ms_prepass = run.ev.ms;
        stats->render_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - run.t0).count();
    }
    *out = set.release();
    return RL_OK;
}
// One lane per iteration (k_plane_generate_lanes): the serial call's checks, then the lanes; a redraw anywhere hands the whole call to the serial kernel
extern "C" int rl_plane_generate_lanes(rl_context* ctx, uint32_t nb_primitive, int strategy, rl_sampler* sampler, rl_plane_set** out, rl_render_stats* stats) {
    if (!ctx || !sampler || !out) return RL_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (strategy < RL_PLANE_STRATEGY_UV || strategy > RL_PLANE_STRATEGY_CMIS) { rl_set_error("strategy must be one of RL_PLANE_STRATEGY_*"); return RL_ERR_INVALID_ARGUMENT; }
    if (nb_primitive == 0 || nb_primitive > (uint32_t)RL_VPL_MAX) { rl_set_error("nb_primitive must be 1 .. RL_VPL_MAX"); return RL_ERR_INVALID_ARGUMENT; }
    int rcode;
    if ((rcode = check_plane_scene(ctx)) != RL_OK) return rcode;
    HIP_OK(hipSetDevice(ctx->device));
    const std::vector<PlaneLight> lights = plane_lights(ctx);
    const unsigned per = (strategy == RL_PLANE_STRATEGY_AVERAGE || strategy == RL_PLANE_STRATEGY_DISCRETE_MIS) ? 3u : 1u, draws = 1u + 6u * per;
    const unsigned n_gen = (nb_primitive + per - 1u) / per, n_planes = n_gen * per;      // n_gen * draws < 2^32: rng_advance's range
    auto set = std::make_unique<rl_plane_set>();
    set->ctx = ctx; set->device = ctx->device;
    HipBuffer<PlaneLight> d_lights;
    if ((rcode = set->d_words.ensure((size_t)n_planes * RL_PLANE_WORDS)) != RL_OK || (rcode = d_lights.ensure(lights.size())) != RL_OK) return rcode;
    const hipStream_t st = ctx->stream;
    HIP_OK(hipMemcpyAsync(d_lights.get(), lights.data(), lights.size() * sizeof(PlaneLight), hipMemcpyHostToDevice, st));
    PlaneGenConst gc{};
    gc.nb_primitive = nb_primitive; gc.cap = n_planes; gc.strategy = strategy;
    gc.n_lights = (unsigned)lights.size(); gc.lights = d_lights.get();
    for (int k = 0; k < 3; k++) { gc.sigma_t[k] = ctx->ds.medium.sigma_t[k]; gc.sigma_s[k] = ctx->ds.medium.sigma_s[k]; }
    gc.words = set->d_words.get();
    LaneRun run;
    if ((rcode = run_one_lane(st, stats != nullptr && !ctx->knobs.has(K_NO_EVENTS), sampler, PLANE_LANES_WORDS, &run, [&](unsigned long long* d_gen) {
            gc.gen_state = d_gen; gc.gen_out = d_gen + 4;
            launch_plane_generate_lanes(st, gc, n_gen);
        })) != RL_OK) return rcode;
    const unsigned long long flag = run.words[4 + PLANE_LANES_FLAG];
    if (flag & 1u) return plane_generate_serial(ctx, nb_primitive, strategy, sampler, out, stats);      // a direction was drawn again: the stream is the serial walk's alone
    if (flag & 2u) { rl_set_error("a plane corner is not finite"); return RL_ERR_INVALID_ARGUMENT; }
    set->on_device = true;
    set->n_planes = n_planes; set->n_gen = n_gen; set->strategy = strategy;
    for (int i = 0; i < 4; i++) sampler->s[i] = run.words[4 + i];
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->camera_samples = n_gen; stats->vertices = n_planes; stats->rng_draws = (uint64_t)n_gen * draws;
        stats->iterations = 1; stats->kernel_launches = 1; stats->ms_prepass = run.ev.ms;
        stats->render_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - run.t0).count();
    }
    *out = set.release();
    return RL_OK;
}
extern "C" int rl_plane_info(const rl_plane_set* set, uint64_t* n_planes, uint64_t* number_plane_gen, int* strategy) {
    if (!set) return RL_ERR_INVALID_ARGUMENT;
    if (n_planes) *n_planes = set->n_planes;
    if (number_plane_gen) *number_plane_gen = set->n_gen;
    if (strategy) *strategy = set->strategy;
    return RL_OK;
}
extern "C" int rl_plane_read(const rl_plane_set* set, uint32_t* words, size_t n_words) {
    if (!set || !words || n_words != (size_t)set->n_planes * RL_PLANE_WORDS) return RL_ERR_INVALID_ARGUMENT;
    const int rcode = set->host_words();
    if (rcode != RL_OK) return rcode;
    std::copy(set->words.begin(), set->words.end(), words);
    return RL_OK;
}
extern "C" void rl_plane_destroy(rl_plane_set* set) {
    if (!set) return;
    if (set->on_device) (void)hipSetDevice(set->device);
    delete set;
}
extern "C" int rl_plane_map_build(rl_context* ctx, const rl_plane_set* set, rl_plane_map** out) {
    if (ctx && knob_on(ctx, K_PLANE_TREE_DEVICE)) return rl_plane_map_build_device(ctx, set, out, nullptr);
    if (!ctx || !set || !out) return RL_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int rcode;
    if ((rcode = check_plane_scene(ctx)) != RL_OK) return rcode;
    if (set->ctx != ctx) { rl_set_error("the plane set belongs to another context"); return RL_ERR_INVALID_ARGUMENT; }
    if ((rcode = set->host_words()) != RL_OK) return rcode;
    ElementTree tree;
    if ((rcode = build_plane_tree(set->words.data(), (size_t)set->n_planes, &tree)) != RL_OK) return rcode;
    const size_t n_nodes = tree.n_nodes(), n_planes = (size_t)set->n_planes;
    const std::vector<float4> h_nodes = pack_tree_nodes(tree);
    std::vector<float4> h_planes(4 * n_planes);
    for (size_t i = 0; i < n_planes; i++) {
        const uint32_t* w = &set->words[(size_t)tree.order[i] * RL_PLANE_WORDS];
        float f[14];
        std::memcpy(f, w, sizeof f);                                   // o, d0, d1, length0, length1, weight
        const uint32_t tb = w[16] | w[17] << 2;
        float ft;
        std::memcpy(&ft, &tb, sizeof ft);
        h_planes[4 * i] = make_float4(f[0], f[1], f[2], f[9]);
        h_planes[4 * i + 1] = make_float4(f[3], f[4], f[5], f[10]);
        h_planes[4 * i + 2] = make_float4(f[6], f[7], f[8], ft);
        h_planes[4 * i + 3] = make_float4(f[11], f[12], f[13], 0.0f);
    }
    const std::vector<PlaneLight> lights = plane_lights(ctx);
    HIP_OK(hipSetDevice(ctx->device));
    auto map = std::make_unique<rl_plane_map>();
    map->ctx = ctx; map->device = ctx->device;
    if ((rcode = map->nodes.ensure(h_nodes.size())) != RL_OK || (rcode = map->planes.ensure(h_planes.size())) != RL_OK || (rcode = map->lights.ensure(lights.size())) != RL_OK) return rcode;
    HIP_OK(hipMemcpy(map->nodes.get(), h_nodes.data(), h_nodes.size() * sizeof(float4), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(map->planes.get(), h_planes.data(), h_planes.size() * sizeof(float4), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(map->lights.get(), lights.data(), lights.size() * sizeof(PlaneLight), hipMemcpyHostToDevice));
    map->n_planes = n_planes; map->n_nodes = n_nodes; map->n_gen = set->n_gen; map->n_lights = lights.size(); map->strategy = set->strategy;
    *out = map.release();
    return RL_OK;
}
// The device build (kernels/planetree.hip): the same map from kernels alone.  plane_tree_run's prepass stands for check_plane_records.
static unsigned plane_tree_group(const rl_context* ctx) {
    if (!ctx->knobs.has(K_PLANE_TREE_GROUP_PLANES)) return (unsigned)RL_PLANE_TREE_GROUP_PLANES;
    return (unsigned)std::min<long long>(std::max<long long>(4, ctx->knobs.i(K_PLANE_TREE_GROUP_PLANES, 0)), RL_PLANE_TREE_GROUP_PLANES);
}
extern "C" int rl_plane_map_build_device(rl_context* ctx, const rl_plane_set* set, rl_plane_map** out, float* ms_kernels) {
    if (!ctx || !set || !out) return RL_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (ms_kernels) *ms_kernels = 0.0f;
    int rcode;
    if ((rcode = check_plane_scene(ctx)) != RL_OK) return rcode;
    if (set->ctx != ctx) { rl_set_error("the plane set belongs to another context"); return RL_ERR_INVALID_ARGUMENT; }
    if (set->n_planes > kElementTreeMax) { rl_set_error("too many planes"); return RL_ERR_INVALID_ARGUMENT; }
    HIP_OK(hipSetDevice(ctx->device));
    const unsigned n = (unsigned)set->n_planes, n_nodes = photon_tree_node_count(n);
    HipBuffer<unsigned> uploaded;                     // a set made on the host: its one upload
    const unsigned* d_words = set->d_words.get();
    if (!set->on_device) {
        if ((rcode = uploaded.ensure(set->words.size())) != RL_OK) return rcode;
        HIP_OK(hipMemcpyAsync(uploaded.get(), set->words.data(), set->words.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        d_words = uploaded.get();
    }
    const std::vector<PlaneLight> lights = plane_lights(ctx);
    auto map = std::make_unique<rl_plane_map>();
    map->ctx = ctx; map->device = ctx->device;
    if ((rcode = map->nodes.ensure(2 * (size_t)n_nodes)) != RL_OK || (rcode = map->planes.ensure(4 * (size_t)n)) != RL_OK || (rcode = map->lights.ensure(lights.size())) != RL_OK) return rcode;
    HIP_OK(hipMemcpyAsync(map->lights.get(), lights.data(), lights.size() * sizeof(PlaneLight), hipMemcpyHostToDevice, ctx->stream));
    const PlaneTreeJob job{d_words, n, plane_tree_group(ctx), map->nodes.get(), nullptr, map->planes.get()};
    if ((rcode = plane_tree_run(job, ctx->stream, !ctx->knobs.has(K_NO_EVENTS), ms_kernels)) != RL_OK) return rcode;      // returns synchronised: `lights` and `uploaded` may go
    map->n_planes = n; map->n_nodes = n_nodes; map->n_gen = set->n_gen; map->n_lights = lights.size(); map->strategy = set->strategy;
    *out = map.release();
    return RL_OK;
}
extern "C" int rl_plane_tree_build_device(rl_context* ctx, const uint32_t* words, size_t n_planes, size_t node_capacity, size_t* n_nodes, float* node_boxes,
                                          uint32_t* node_links, uint32_t* order) {
    if (!ctx || !n_nodes || (n_planes && !words)) return RL_ERR_INVALID_ARGUMENT;
    int rcode;
    if (n_planes > kElementTreeMax) { rl_set_error("too many planes"); return RL_ERR_INVALID_ARGUMENT; }      // before any allocation
    const bool size_only = !node_boxes && !node_links && !order;
    if (n_planes == 0) { *n_nodes = 0; return RL_OK; }
    HIP_OK(hipSetDevice(ctx->device));
    const unsigned n = (unsigned)n_planes, count = photon_tree_node_count(n);
    HipBuffer<unsigned> d_words, d_order;
    HipBuffer<float4> d_nodes;
    if ((rcode = d_words.ensure(n_planes * RL_PLANE_WORDS)) != RL_OK) return rcode;
    HIP_OK(hipMemcpyAsync(d_words.get(), words, n_planes * RL_PLANE_WORDS * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    if (size_only || node_capacity < count || !node_boxes || !node_links || !order) {
        // the host build refuses a bad record before it looks at the capacity or the arrays: the prepass alone
        const PlaneTreeJob check{d_words.get(), n, plane_tree_group(ctx), nullptr, nullptr, nullptr};
        if ((rcode = plane_tree_run(check, ctx->stream, false, nullptr)) != RL_OK) return rcode;
        *n_nodes = count;
        if (size_only) return RL_OK;
        if (node_capacity < count) rl_set_error("rl_plane_tree_build_device: node_capacity is too small");
        return RL_ERR_INVALID_ARGUMENT;
    }
    if ((rcode = d_order.ensure(n)) != RL_OK || (rcode = d_nodes.ensure(2 * (size_t)count)) != RL_OK) return rcode;
    const PlaneTreeJob job{d_words.get(), n, plane_tree_group(ctx), d_nodes.get(), d_order.get(), nullptr};
    if ((rcode = plane_tree_run(job, ctx->stream, false, nullptr)) != RL_OK) return rcode;
    *n_nodes = count;
    std::vector<float4> h_nodes(2 * (size_t)count);
    HIP_OK(hipMemcpy(h_nodes.data(), d_nodes.get(), h_nodes.size() * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(order, d_order.get(), (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    unpack_tree_nodes(h_nodes, count, node_boxes, node_links);
    return RL_OK;
}
extern "C" int rl_plane_map_info(const rl_plane_map* map, uint64_t* n_planes, uint64_t* n_nodes, uint64_t* number_plane_gen, int* strategy) {
    if (!map) return RL_ERR_INVALID_ARGUMENT;
    if (n_planes) *n_planes = map->n_planes;
    if (n_nodes) *n_nodes = map->n_nodes;
    if (number_plane_gen) *number_plane_gen = map->n_gen;
    if (strategy) *strategy = map->strategy;
    return RL_OK;
}
extern "C" int rl_plane_map_read(const rl_plane_map* map, size_t node_capacity, float* node_boxes, uint32_t* node_links, size_t plane_capacity, float* planes) {
    if (!map || !node_boxes || !node_links || !planes) return RL_ERR_INVALID_ARGUMENT;
    if (node_capacity < map->n_nodes || plane_capacity < map->n_planes) { rl_set_error("rl_plane_map_read: a capacity is too small"); return RL_ERR_INVALID_ARGUMENT; }
    HIP_OK(hipSetDevice(map->device));
    return read_tree(map->nodes, (size_t)map->n_nodes, map->planes, (size_t)map->n_planes * 4, node_boxes, node_links, planes);
}
extern "C" void rl_plane_map_destroy(rl_plane_map* map) { destroy_handle(map); }
extern "C" int rl_render_plane_single(rl_context* ctx, const rl_plane_map* map, uint32_t spp, int32_t seed_variant, uint32_t shard_index, uint32_t shard_count,
                                      const uint64_t* block_seeds, size_t n_blocks, float* out_rgb, rl_render_stats* stats) {
    if (!map) return RL_ERR_INVALID_ARGUMENT;
    static const GatherKind kind{"plane-single", "plane map", check_plane_scene, 2, {STAT_PLANE_ISECT, STAT_PLANE_VISIBLE}, {STAT_PLANE_ISECT_HI, STAT_PLANE_VISIBLE_HI}};
    const int rcode = render_gather(ctx, kind, map->ctx, spp, seed_variant, shard_index, shard_count, block_seeds, n_blocks, out_rgb, stats,
                                    [&](bool lds_scene, dim3 grid, size_t lds, hipStream_t st, const RenderConst& rc, const StackConf& stc) {
        PlaneConst pc{};
        pc.nodes = map->nodes.get(); pc.planes = map->planes.get(); pc.lights = map->lights.get(); pc.n_nodes = (unsigned)map->n_nodes;
        pc.w = map->strategy == RL_PLANE_STRATEGY_AVERAGE ? 1.0f / 3.0f : 1.0f;
        pc.n_lights_f = (float)map->n_lights;                                   // emitters.len() as f32
        pc.inv_gen = 1.0f / (float)map->n_gen;                                  // 1.0 / number_plane_gen as f32
        const int mode = map->strategy == RL_PLANE_STRATEGY_DISCRETE_MIS ? PLANE_MODE_DISCRETE_MIS : map->strategy == RL_PLANE_STRATEGY_CMIS ? PLANE_MODE_CMIS : PLANE_MODE_PLAIN;
        (lds_scene ? launch_plane_lds : launch_plane_stream)(mode, grid, dim3(256), lds, st, rc, ctx->ds, stc, pc);
    });
    if (rcode == RL_OK && stats) stats->shadow_rays = stats->reserved[1];      // reserved[1] = planes intersected, each of which takes a visibility ray; [2] = of those visible
    return rcode;
}

// ---- IntegratorSinglePlaneUncorrelated (uncorrelated_plane_single.rs): no plane pass and no map — every camera sample makes its nb_primitive planes itself
// (k_uplane, uplane.hip.h); the call uploads the rectangular lights and launches once.  reserved[0], the gather's nodes entered, carries the direction redraws.
extern "C" int rl_render_plane_uncorrelated(rl_context* ctx, uint32_t nb_primitive, int strategy, uint32_t spp, int32_t seed_variant, uint32_t shard_index, uint32_t shard_count,
                                            const uint64_t* block_seeds, size_t n_blocks, float* out_rgb, rl_render_stats* stats) {
    if (!ctx) return RL_ERR_INVALID_ARGUMENT;
    if (strategy < RL_PLANE_STRATEGY_UV || strategy > RL_PLANE_STRATEGY_CMIS) { rl_set_error("strategy must be one of RL_PLANE_STRATEGY_*"); return RL_ERR_INVALID_ARGUMENT; }
    if (nb_primitive == 0 || nb_primitive > (uint32_t)RL_VPL_MAX) { rl_set_error("nb_primitive must be 1 .. RL_VPL_MAX"); return RL_ERR_INVALID_ARGUMENT; }
    const bool pick = strategy == RL_PLANE_STRATEGY_AVERAGE || strategy == RL_PLANE_STRATEGY_DISCRETE_MIS;
    const uint64_t draws = 2ull + (uint64_t)nb_primitive * (pick ? 8u : 7u);      // the jitter; per plane id_emitter, the type (Average / DiscreteMIS), plane_sample's 6
    const GatherKind kind{"plane-single --uncorrelated", "context", check_plane_scene, 2, {STAT_PLANE_ISECT, STAT_PLANE_VISIBLE}, {STAT_PLANE_ISECT_HI, STAT_PLANE_VISIBLE_HI}, draws};
    int rcode;
    if ((rcode = check_frame(ctx, spp, block_seeds, n_blocks, out_rgb)) != RL_OK || (rcode = check_plane_scene(ctx)) != RL_OK) return rcode;
    HIP_OK(hipSetDevice(ctx->device));
    const std::vector<PlaneLight> lights = plane_lights(ctx);
    HipBuffer<PlaneLight> d_lights;               // freed once render_gather has synchronised
    if ((rcode = d_lights.ensure(lights.size())) != RL_OK) return rcode;
    HIP_OK(hipMemcpy(d_lights.get(), lights.data(), lights.size() * sizeof(PlaneLight), hipMemcpyHostToDevice));
    rcode = render_gather(ctx, kind, ctx, spp, seed_variant, shard_index, shard_count, block_seeds, n_blocks, out_rgb, stats,
                          [&](bool lds_scene, dim3 grid, size_t lds, hipStream_t st, const RenderConst& rc, const StackConf& stc) {
        UPlaneConst uc{};
        uc.lights = d_lights.get(); uc.n_lights = (unsigned)lights.size();
        uc.nb_primitive = nb_primitive; uc.draws = (unsigned)draws;
        uc.pick_type = pick ? 1 : 0;
        uc.type = strategy == RL_PLANE_STRATEGY_UV ? RL_PLANE_UV : strategy == RL_PLANE_STRATEGY_VT ? RL_PLANE_VT : strategy == RL_PLANE_STRATEGY_UT ? RL_PLANE_UT : RL_PLANE_UALPHAT;
        uc.w = strategy == RL_PLANE_STRATEGY_AVERAGE ? 1.0f / 3.0f : 1.0f;
        uc.n_lights_f = (float)lights.size();                                   // rect_lights.len() as f32
        uc.inv_nb = 1.0f / (float)nb_primitive;                                 // 1.0 / self.nb_primitive as f32
        const int mode = strategy == RL_PLANE_STRATEGY_DISCRETE_MIS ? PLANE_MODE_DISCRETE_MIS : strategy == RL_PLANE_STRATEGY_CMIS ? PLANE_MODE_CMIS : PLANE_MODE_PLAIN;
        (lds_scene ? launch_uplane_lds : launch_uplane_stream)(mode, grid, dim3(256), lds, st, rc, ctx->ds, stc, uc);
    });
    if (rcode == RL_OK && stats) {
        stats->shadow_rays = stats->reserved[1];                                // each plane the ray meets takes one visibility ray
        stats->rng_draws = stats->camera_samples * draws + 2 * stats->reserved[0];
    }
    return rcode;
}
