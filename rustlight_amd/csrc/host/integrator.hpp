// integrator.hpp — C++ mirror of the reference's plugin surface for the `path` hot path, layered
// on the C-ABI (include/rustlight_amd.h).  Names, argument meaning and defaults follow rustlight:
//   trait Sampler / IndependentSampler      src/samplers/mod.rs:3-9, independent.rs:5-34
//   struct Scene                            src/scene.rs:16-30
//   struct BufferCollection ("primal")      src/integrators/mod.rs:48-216
//   trait Integrator::compute               src/integrators/mod.rs:219-233
//   struct IntegratorPathTracing            src/integrators/explicit/path.rs:14-20
//   IntegratorType::compute (BVH build is untimed, then "Elapsed Integrator")  mod.rs:274-338
#pragma once
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../../include/rustlight_amd.h"

namespace rustlight {

struct IndependentSampler {   // owns the concrete SmallRng so the raw u64 stream is reachable
    rl_sampler rnd;
    int variant = 0;
    explicit IndependentSampler(uint64_t seed, int variant_ = 0) : variant(variant_) { rl_sampler_seed(&rnd, seed, variant_); }
    float next() { return rl_sampler_next_f32(&rnd); }
    uint64_t next_u64() { return rl_sampler_next_u64(&rnd); }
};

struct Scene {
    rl_scene* handle = nullptr;
    size_t nb_samples = 1;           // Scene::nb_samples (CLI global -n)
    std::string output_img_path = "out.pfm";
    explicit Scene(rl_scene* h) : handle(h) {}
    Scene(const Scene&) = delete;
    Scene& operator=(const Scene&) = delete;
    ~Scene() { rl_scene_destroy(handle); }
    static Scene* load(const std::string& path, bool use_shading_normals = true) {
        rl_scene* h = nullptr;
        int rc = rl_scene_load(path.c_str(), use_shading_normals ? 1 : 0, &h);   // SceneLoaderManager: .pbrt | .xml
        if (rc != RL_OK) throw std::runtime_error(std::string("error on loading the scene: ") + rl_last_error());
        return new Scene(h);
    }
    void build_emitters(bool build_ats = false) {   // Scene::build_emitters(build_ats) (scene.rs:53-123)
        if (rl_scene_enable_ats(handle, build_ats ? 1 : 0) != RL_OK || rl_scene_build_emitters(handle) != RL_OK)
            throw std::runtime_error(std::string("build_emitters failed: ") + rl_last_error());
    }
};

struct BufferCollection {   // only the "primal" buffer exists on this path
    uint32_t width = 0, height = 0;
    std::vector<float> primal;   // W*H*3, row-major, origin top-left
    void save(const std::string& /*name = "primal"*/, const std::string& path) const {   // Bitmap::save: .pfm | .png | .exr
        if (rl_save_image(path.c_str(), primal.data(), width, height) != RL_OK) throw std::runtime_error("cannot write " + path);
    }
    void scale(float v) { for (float& x : primal) x *= v; }                                   // Bitmap::scale
    void accumulate_bitmap(const BufferCollection& o) { for (size_t i = 0; i < primal.size(); i++) primal[i] += o.primal[i]; }
};

// ---- what every integrator's compute() does around its own ABI calls, written once
using Options = std::vector<std::pair<std::string, std::string>>;   // execution options of a device context: `rustlight-amd --option name=value`
inline void check(int rc, const char* what) {   // "<what>: <the library's message>"
    if (rc != RL_OK) throw std::runtime_error(std::string(what) + ": " + rl_last_error());
}
// the ABI's handles, destroyed with their owner: also when what runs after their creation throws
template <class T, void (*Destroy)(T*)> struct HandleDeleter { void operator()(T* h) const { Destroy(h); } };
template <class T, void (*Destroy)(T*)> using Handle = std::unique_ptr<T, HandleDeleter<T, Destroy>>;
using ContextHandle = Handle<rl_context, rl_context_destroy>;
using VplSetHandle = Handle<rl_vpl_set, rl_vpl_destroy>;
inline ContextHandle create_context(const Scene& scene, int device) {
    rl_context* c = nullptr;
    check(rl_context_create(scene.handle, device, &c), "rl_context_create");
    return ContextHandle(c);
}
// `named`: the message names the option ("--option NAME: ...") instead of the call
inline void apply_options(rl_context* c, const Options& options, bool named) {
    for (const auto& o : options) check(rl_context_set_option(c, o.first.c_str(), o.second.c_str()), (named ? "--option " + o.first : std::string("rl_context_set_option")).c_str());
}
inline BufferCollection zeroed_image(const Scene& scene) {
    BufferCollection img;
    rl_scene_image_size(scene.handle, &img.width, &img.height);
    img.primal.assign((size_t)3 * img.width * img.height, 0.0f);
    return img;
}
inline std::vector<uint64_t> draw_block_seeds(IndependentSampler& sampler, const BufferCollection& img) {   // generate_img_blocks
    std::vector<uint64_t> seeds(rl_block_count(img.width, img.height));
    rl_generate_block_seeds(&sampler.rnd, img.width, img.height, seeds.data(), seeds.size());
    return seeds;
}
// One render's device context: created on (scene, device) with the options applied, destroyed with the render; img is the zeroed image of the scene's size
struct RenderContext {
    ContextHandle ctx;
    BufferCollection img;
    RenderContext(const Scene& scene, int device, const Options& options = {}) : ctx(create_context(scene, device)) {
        apply_options(ctx.get(), options, true);
        img = zeroed_image(scene);
    }
    operator rl_context*() const { return ctx.get(); }
    std::vector<uint64_t> block_seeds(IndependentSampler& sampler) const { return draw_block_seeds(sampler, img); }
};

enum class IntegratorPathTracingStrategies { All = RL_STRATEGY_ALL, BSDF = RL_STRATEGY_BSDF, Emitter = RL_STRATEGY_EMITTER };

struct IntegratorPathTracing {
    std::optional<uint32_t> min_depth = 0, max_depth = std::nullopt, rr_depth = 0;
    IntegratorPathTracingStrategies strategy = IntegratorPathTracingStrategies::All;
    bool single_scattering = false;
    // MI355X-specific knobs (not in the reference)
    int device = 0;
    // RL_STREAM_REFERENCE_ORDER = rustlight's own stream assignment (seed-for-seed the reference's image); RL_STREAM_PER_SAMPLE is the
    // throughput decomposition (statistically the same image, ~5x faster on the Cornell box at 1080p x 128 spp since round 4): opt-in
    rl_stream_mode stream_mode = RL_STREAM_REFERENCE_ORDER;
    uint32_t numerics = RL_NUMERICS_EXACT;      // RL_NUMERICS_FAST: opt-in tolerance mode
    uint32_t shard_index = 0, shard_count = 1;
    rl_render_stats last_stats{};

    // several GPUs of one node from one process (the CLI's --gpus N): GPU g renders the blocks b % N == g on its
    // own host thread into its own framebuffer in HBM; ONE ncclReduce over xGMI merges them on the first GPU (rl_multi_*)
    int n_gpus = 1;

    // frames in flight (one GPU): how many independent frames `compute_frames` — and the progressive wrappers through it — keep on the GPU at once, one device
    // context and one host thread each.  A frame's render is a chain of dependent launches that leaves much of the chip idle at its tail (reference-order
    // streams: the chain pass ends with its slowest wave); another context's frame fills it.  The images are those of one frame after the other.
    int frames_in_flight = 1;

    // execution options handed to every device context this integrator creates (Options above: test / measurement hooks, none changes an image;
    // e.g. {"spec_draws_per_sample", "40"}); `rustlight-amd --option name=value`
    Options options;
    void apply_options(rl_context* c) const { rustlight::apply_options(c, options, false); }

    // the device contexts (BVH + uploaded scene) are built once per scene, like `BVHAccel::new` in IntegratorType::compute
    rl_context* ctx = nullptr;
    std::vector<rl_context*> extra_ctx;      // frames in flight: contexts 2 .. frames_in_flight
    rl_multi* multi = nullptr;
    const Scene* ctx_scene = nullptr;
    int ctx_gpus = 0;
    IntegratorPathTracing() = default;
    IntegratorPathTracing(const IntegratorPathTracing&) = delete;
    ~IntegratorPathTracing() { release(); }
    void release() {
        if (ctx) rl_context_destroy(ctx);
        for (rl_context* c : extra_ctx) rl_context_destroy(c);
        extra_ctx.clear();
        if (multi) rl_multi_destroy(multi);
        ctx = nullptr; multi = nullptr;
    }
    rl_path_params params_for(const IndependentSampler& sampler, const Scene& scene) const {
        rl_path_params p;
        rl_path_params_default(&p);
        p.spp = (uint32_t)scene.nb_samples;
        p.has_min_depth = min_depth.has_value(); p.min_depth = min_depth.value_or(0);
        p.has_max_depth = max_depth.has_value(); p.max_depth = max_depth.value_or(0);
        p.has_rr_depth = rr_depth.has_value(); p.rr_depth = rr_depth.value_or(0);
        p.strategy = (int)strategy;
        p.single_scattering = single_scattering;
        p.stream_mode = stream_mode;
        p.numerics = numerics;
        p.seed_variant = sampler.variant;
        p.shard_index = shard_index; p.shard_count = shard_count;
        return p;
    }

    // `n_frames` consecutive compute() calls with up to `frames_in_flight` of them on the GPU at once: the block seeds of every frame are drawn from the master
    // sampler in call order (exactly what that many sequential calls draw), frame j renders on context j % k from host thread j % k; images in frame order.
    std::vector<BufferCollection> compute_frames(IndependentSampler& sampler, Scene& scene, size_t n_frames) {
        std::vector<BufferCollection> out;
        const size_t k = std::min<size_t>((size_t)std::max(1, frames_in_flight), std::max<size_t>(1, n_frames));
        if (k <= 1 || std::max(1, n_gpus) > 1) {
            for (size_t j = 0; j < n_frames; j++) out.push_back(compute(sampler, scene));
            return out;
        }
        if (ctx_scene != &scene || ctx_gpus != 1 || !ctx) {
            release();
            ctx = create_context(scene, device).release();
            apply_options(ctx);
            ctx_scene = &scene; ctx_gpus = 1;
        }
        while (extra_ctx.size() + 1 < k) {
            extra_ctx.push_back(create_context(scene, device).release());
            apply_options(extra_ctx.back());
        }
        const rl_path_params p = params_for(sampler, scene);
        out.resize(n_frames);
        std::vector<std::vector<uint64_t>> seeds(n_frames);
        for (size_t j = 0; j < n_frames; j++) {
            out[j] = zeroed_image(scene);
            seeds[j] = draw_block_seeds(sampler, out[j]);   // in frame order
        }
        std::vector<std::string> errors(k);
        std::vector<rl_render_stats> stats(k);
        std::vector<std::thread> threads;
        for (size_t c = 0; c < k; c++)
            threads.emplace_back([&, c]() {
                rl_context* cx = c == 0 ? ctx : extra_ctx[c - 1];
                for (size_t j = c; j < n_frames; j += k) {
                    if (rl_render_path(cx, &p, seeds[j].data(), seeds[j].size(), out[j].primal.data(), 0, nullptr, &stats[c]) != RL_OK) { errors[c] = rl_last_error(); return; }   // (the error string is per thread)
                }
            });
        for (std::thread& t : threads) t.join();
        for (const std::string& e : errors) if (!e.empty()) throw std::runtime_error("rl_render_path: " + e);
        last_stats = stats[(n_frames - 1) % k];
        return out;
    }

    // IntegratorType::compute + Integrator::compute: builds the BVH (untimed, first call), renders, returns the image
    BufferCollection compute(IndependentSampler& sampler, Scene& scene) {
        const int n = std::max(1, n_gpus);
        if (ctx_scene != &scene || ctx_gpus != n || (!ctx && !multi)) {
            release();
            if (n == 1) {
                ctx = create_context(scene, device).release();
                apply_options(ctx);
            } else {
                int n_dev = 0;
                rl_device_count(&n_dev);
                std::vector<int> devs(n);
                for (int g = 0; g < n; g++) devs[g] = n_dev > 0 ? (device + g) % n_dev : device + g;
                check(rl_multi_create(scene.handle, devs.data(), n, &multi), "rl_multi_create");
            }
            ctx_scene = &scene; ctx_gpus = n;
        }
        BufferCollection img = zeroed_image(scene);
        rl_path_params p = params_for(sampler, scene);
        const std::vector<uint64_t> seeds = draw_block_seeds(sampler, img);
        if (n == 1) {
            check(rl_render_path(ctx, &p, seeds.data(), seeds.size(), img.primal.data(), 0, nullptr, &last_stats), "rl_render_path");
            return img;
        }
        p.shard_index = 0; p.shard_count = 1;      // (rl_multi deals the blocks itself)
        check(rl_multi_render_path(multi, &p, seeds.data(), seeds.size(), img.primal.data(), &last_stats), "rl_multi_render_path");
        return img;
    }
};

// struct IntegratorAO (src/integrators/ao.rs:4-7) / struct IntegratorDirect (src/integrators/direct.rs:5-8)
struct IntegratorMC {
    int device = 0;
    rl_stream_mode stream_mode = RL_STREAM_REFERENCE_ORDER;
    rl_render_stats last_stats{};
  protected:
    BufferCollection run(bool direct, rl_mc_params p, IndependentSampler& sampler, Scene& scene) {
        RenderContext ctx(scene, device);
        p.spp = (uint32_t)scene.nb_samples;
        p.stream_mode = stream_mode;
        p.seed_variant = sampler.variant;
        p.shard_index = 0; p.shard_count = 1;
        const std::vector<uint64_t> seeds = ctx.block_seeds(sampler);
        check((direct ? rl_render_direct : rl_render_ao)(ctx, &p, seeds.data(), seeds.size(), ctx.img.primal.data(), 0, nullptr, &last_stats), "render");
        return std::move(ctx.img);
    }
};
struct IntegratorAO : IntegratorMC {
    std::optional<float> max_distance = 1.0f;
    bool normal_correction = false;
    BufferCollection compute(IndependentSampler& sampler, Scene& scene) {
        rl_mc_params p{};
        p.has_max_distance = max_distance.has_value(); p.max_distance = max_distance.value_or(0.0f);
        p.normal_correction = normal_correction;
        return run(false, p, sampler, scene);
    }
};
struct IntegratorDirect : IntegratorMC {
    size_t nb_bsdf_samples = 1, nb_light_samples = 1;
    BufferCollection compute(IndependentSampler& sampler, Scene& scene) {
        rl_mc_params p{};
        p.nb_bsdf_samples = (uint32_t)nb_bsdf_samples; p.nb_light_samples = (uint32_t)nb_light_samples;
        return run(true, p, sampler, scene);
    }
};

// struct IntegratorLightTracing (src/integrators/explicit/light.rs:7-13): light paths splatted through the camera, on per-sample streams (rl_render_light)
struct IntegratorLightTracing {
    std::optional<uint32_t> max_depth, min_depth, rr_depth;
    rl_light_strategy strategy = RL_LIGHT_ALL;     // all | surface | volume: render_surface / render_volume
    int device = 0;
    Options options;
    rl_render_stats last_stats{};
    BufferCollection compute(IndependentSampler& sampler, Scene& scene) {
        RenderContext ctx(scene, device, options);
        rl_path_params p;
        rl_path_params_default(&p);
        p.spp = (uint32_t)scene.nb_samples;
        p.has_min_depth = min_depth.has_value(); p.min_depth = min_depth.value_or(0);
        p.has_max_depth = max_depth.has_value(); p.max_depth = max_depth.value_or(0);
        p.has_rr_depth = rr_depth.has_value(); p.rr_depth = rr_depth.value_or(0);
        p.strategy = strategy;
        p.stream_mode = RL_STREAM_PER_SAMPLE;
        p.seed_variant = sampler.variant;
        const std::vector<uint64_t> seeds = ctx.block_seeds(sampler);
        check(rl_render_light(ctx, &p, seeds.data(), seeds.size(), ctx.img.primal.data(), 0, nullptr, &last_stats), "render");
        return std::move(ctx.img);
    }
};

// How the light paths of IntegratorVPL / IntegratorVolPrimitives draw.  Reference: rl_vpl_generate, one lane on the main sampler's serial stream, seed for seed
// the reference (the default).  PerPath: rl_vpl_generate_paths, one light path per lane on the stream of the k-th clone_box of the main sampler — statistically,
// not seed-for-seed, the same image (`--light-streams per-path`).  The gather is the same either way.
enum class LightStreams { Reference, PerPath };
inline VplSetHandle generate_light_records(LightStreams streams, rl_context* ctx, const rl_path_params& p, uint32_t n, rl_vpl_option option, IndependentSampler& sampler,
                                           rl_render_stats* stats, const char* who) {
    rl_vpl_set* set = nullptr;
    check((streams == LightStreams::PerPath ? rl_vpl_generate_paths : rl_vpl_generate)(ctx, &p, n, option, &sampler.rnd, &set, stats), who);
    return VplSetHandle(set);
}
// struct IntegratorVPL (src/integrators/explicit/vpl.rs:16-23) + Integrator::compute, seed for seed the reference: the VPLs from the main sampler
// (rl_vpl_generate), the block seeds from the sampler it leaves, the gather on reference-order streams (rl_render_vpl).  clamping_factor is not a
// field: the reference never reads it.
struct IntegratorVPL {
    uint32_t nb_vpl = 128;
    std::optional<uint32_t> max_depth, rr_depth = 0u;
    rl_vpl_option option_vpl = RL_VPL_ALL, option_lt = RL_VPL_ALL;
    LightStreams light_streams = LightStreams::Reference;
    int device = 0;
    Options options;
    rl_render_stats last_stats{}, last_generation_stats{};
    BufferCollection compute(IndependentSampler& sampler, Scene& scene) {
        RenderContext ctx(scene, device, options);
        rl_path_params p;
        rl_path_params_default(&p);
        p.spp = (uint32_t)scene.nb_samples;
        p.has_max_depth = max_depth.has_value(); p.max_depth = max_depth.value_or(0);
        p.has_rr_depth = rr_depth.has_value(); p.rr_depth = rr_depth.value_or(0);
        p.stream_mode = RL_STREAM_REFERENCE_ORDER;
        p.seed_variant = sampler.variant;
        const VplSetHandle vpls = generate_light_records(light_streams, ctx, p, nb_vpl, option_vpl, sampler, &last_generation_stats, "vpl");
        const std::vector<uint64_t> seeds = ctx.block_seeds(sampler);
        check(rl_render_vpl(ctx, vpls.get(), &p, option_lt, seeds.data(), seeds.size(), ctx.img.primal.data(), 0, nullptr, &last_stats), "vpl");
        return std::move(ctx.img);
    }
};

// compute of the integrators that gather a map of light-pass records, written once: generate(&set) on the main sampler, build(set, &map), the block seeds from
// the sampler the generation leaves, `render` on reference-order streams into ctx.img.  Set and map are destroyed with the call, also when a later step throws;
// every message stands under `what`.
template <class Set, class Map, class Generate, class Build>
BufferCollection compute_with_map(RenderContext& ctx, IndependentSampler& sampler, const Scene& scene, const char* what, Generate&& generate, void (*destroy_set)(Set*), Build&& build,
                                  void (*destroy_map)(Map*), int (*render)(rl_context*, const Map*, uint32_t, int32_t, uint32_t, uint32_t, const uint64_t*, size_t, float*, rl_render_stats*),
                                  rl_render_stats* last_stats) {
    Set* generated = nullptr;
    check(generate(&generated), what);
    const std::unique_ptr<Set, void (*)(Set*)> set(generated, destroy_set);
    Map* built = nullptr;
    check(build(set.get(), &built), what);
    const std::unique_ptr<Map, void (*)(Map*)> map(built, destroy_map);
    const std::vector<uint64_t> seeds = ctx.block_seeds(sampler);
    check(render(ctx, map.get(), (uint32_t)scene.nb_samples, sampler.variant, 0, 1, seeds.data(), seeds.size(), ctx.img.primal.data(), last_stats), what);
    return std::move(ctx.img);
}
// the light paths' parameters of IntegratorVolPrimitives and the three structs made of it: `self`'s depths, the reference's stream order
template <class Self>
rl_path_params light_path_params(const Self& self, const IndependentSampler& sampler) {
    rl_path_params p;
    rl_path_params_default(&p);
    p.has_max_depth = self.max_depth.has_value(); p.max_depth = self.max_depth.value_or(0);
    p.has_rr_depth = self.rr_depth.has_value(); p.rr_depth = self.rr_depth.value_or(0);
    p.stream_mode = RL_STREAM_REFERENCE_ORDER;
    p.seed_variant = sampler.variant;
    return p;
}

// struct IntegratorVolPrimitives { nb_primitive, max_depth, rr_depth, primitives } (src/integrators/explicit/vol_primitives.rs:12-24) + Integrator::compute
// for the beam radiance estimate, seed for seed the reference: the photons from the main sampler (rl_vpl_generate with RL_VPL_VOLUME: the records convert_photons
// stores), the photon tree (rl_photon_map_build), the block seeds from the sampler the generation leaves, the gather on reference-order streams (rl_render_bre).
// Beams, Planes and VRL are not built here (they are structs of their own, below).  radius: the reference hard-codes 0.001 (vol_primitives.rs:618).  tree_build: Host = rl_photon_map_build (the records
// go to the host and the tree comes back), Device = rl_photon_map_build_device (the same tree, byte for byte, from device kernels; `--tree-build device`).
enum class VolPrimitivies { BRE, Beams, Planes, VRL };
enum class TreeBuild { Host, Device };
struct IntegratorVolPrimitives {
    uint32_t nb_primitive = 128;
    std::optional<uint32_t> max_depth, rr_depth = 0u;
    VolPrimitivies primitives = VolPrimitivies::BRE;
    float radius = RL_PHOTON_RADIUS_DEFAULT;
    LightStreams light_streams = LightStreams::Reference;
    TreeBuild tree_build = TreeBuild::Host;
    int device = 0;
    Options options;
    rl_render_stats last_stats{}, last_generation_stats{};
    BufferCollection compute(IndependentSampler& sampler, Scene& scene) {
        if (primitives != VolPrimitivies::BRE) throw std::runtime_error("vol-primitives: only the beam radiance estimate (bre) is built");
        RenderContext ctx(scene, device, options);
        const rl_path_params p = light_path_params(*this, sampler);
        return compute_with_map(ctx, sampler, scene, "vol-primitives",
            [&](rl_vpl_set** out) { return (light_streams == LightStreams::PerPath ? rl_vpl_generate_paths : rl_vpl_generate)(ctx, &p, nb_primitive, RL_VPL_VOLUME, &sampler.rnd, out, &last_generation_stats); },
            rl_vpl_destroy,
            [&](const rl_vpl_set* photons, rl_photon_map** out) {
                return tree_build == TreeBuild::Device ? rl_photon_map_build_device(ctx, photons, radius, out, nullptr) : rl_photon_map_build(ctx, photons, radius, out);
            },
            rl_photon_map_destroy, rl_render_bre, &last_stats);
    }
};

// compute of the three structs below, which have the same fields: the context, light_path_params, then compute_with_map over the beam or plane pass of
// `self.light_streams` (generate / generate_paths), `build` at self.radius and `render`
template <class Self, class Set, class Map>
BufferCollection compute_beam_pass(Self& self, IndependentSampler& sampler, Scene& scene, const char* what,
                                   int (*generate)(rl_context*, const rl_path_params*, uint32_t, rl_sampler*, Set**, rl_render_stats*), decltype(generate) generate_paths,
                                   void (*destroy_set)(Set*), int (*build)(rl_context*, const Set*, float, Map**), void (*destroy_map)(Map*),
                                   int (*render)(rl_context*, const Map*, uint32_t, int32_t, uint32_t, uint32_t, const uint64_t*, size_t, float*, rl_render_stats*)) {
    RenderContext ctx(scene, self.device, self.options);
    const rl_path_params p = light_path_params(self, sampler);
    return compute_with_map(ctx, sampler, scene, what,
        [&](Set** out) { return (self.light_streams == LightStreams::PerPath ? generate_paths : generate)(ctx, &p, self.nb_primitive, &sampler.rnd, out, &self.last_generation_stats); },
        destroy_set, [&](const Set* set, Map** out) { return build(ctx, set, self.radius, out); }, destroy_map, render, &self.last_stats);
}

// IntegratorVolPrimitives with primitives = Beams (vol_primitives.rs:437-523, 608-790) as a struct of its own — IntegratorVolPrimitives above keeps refusing every
// primitive but BRE, and nothing above refers to this one — + Integrator::compute, seed for seed the reference: the beams from the main sampler
// (rl_beam_generate: the light paths of rl_vpl_generate stored by convert_beams(false, ..)), the split and the beam tree (rl_beam_map_build), the block seeds
// from the sampler the generation leaves, the gather on reference-order streams (rl_render_beams).  light_streams = PerPath: rl_beam_generate_paths.
struct IntegratorPhotonBeams {
    uint32_t nb_primitive = 128;
    std::optional<uint32_t> max_depth, rr_depth = 0u;
    float radius = RL_PHOTON_RADIUS_DEFAULT;
    LightStreams light_streams{LightStreams::Reference};
    int device = 0;
    Options options;
    rl_render_stats last_stats{}, last_generation_stats{};
    BufferCollection compute(IndependentSampler& sampler, Scene& scene) {
        return compute_beam_pass(*this, sampler, scene, "photon-beams", rl_beam_generate, rl_beam_generate_paths, rl_beam_destroy, rl_beam_map_build, rl_beam_map_destroy, rl_render_beams);
    }
};

// IntegratorVolPrimitives with primitives = Planes (vol_primitives.rs:256-435, 608-790) as a struct of its own, for the reason IntegratorPhotonBeams is one, +
// Integrator::compute, seed for seed the reference: the surface beams and the planes from the main sampler (rl_pplane_generate: the light paths of
// rl_beam_generate stored by convert_beams(true, ..) and convert_planes), the split and the two trees (rl_pplane_map_build), the block seeds from the sampler
// the generation leaves, the gather on reference-order streams (rl_render_photon_planes).  light_streams = PerPath: rl_pplane_generate_paths.
struct IntegratorPhotonPlanes {
    uint32_t nb_primitive = 128;
    std::optional<uint32_t> max_depth, rr_depth = 0u;
    float radius = RL_PHOTON_RADIUS_DEFAULT;
    LightStreams light_streams{LightStreams::Reference};
    int device = 0;
    Options options;
    rl_render_stats last_stats{}, last_generation_stats{};
    BufferCollection compute(IndependentSampler& sampler, Scene& scene) {
        return compute_beam_pass(*this, sampler, scene, "photon-planes", rl_pplane_generate, rl_pplane_generate_paths, rl_pplane_destroy, rl_pplane_map_build, rl_pplane_map_destroy,
                                 rl_render_photon_planes);
    }
};

// IntegratorVolPrimitives with primitives = VRL (vol_primitives.rs:201-253, 608-699, 741-764) as a struct of its own, for the reason IntegratorPhotonBeams is one,
// + Integrator::compute, seed for seed the reference: the beams from the main sampler (rl_beam_generate: the VRL arm shoots what the Beams arm shoots), the
// partition by from_surface with the surface beams' split and tree (rl_vrl_map_build), the block seeds from the sampler the generation leaves, the chain pass
// and the gather on reference-order streams (rl_render_vrl).  light_streams = PerPath: rl_beam_generate_paths.
struct IntegratorVirtualRayLights {
    uint32_t nb_primitive = 128;
    std::optional<uint32_t> max_depth, rr_depth = 0u;
    float radius = RL_PHOTON_RADIUS_DEFAULT;
    LightStreams light_streams{LightStreams::Reference};
    int device = 0;
    Options options;
    rl_render_stats last_stats{}, last_generation_stats{};
    BufferCollection compute(IndependentSampler& sampler, Scene& scene) {
        return compute_beam_pass(*this, sampler, scene, "virtual-ray-lights", rl_beam_generate, rl_beam_generate_paths, rl_beam_destroy, rl_vrl_map_build, rl_vrl_map_destroy, rl_render_vrl);
    }
};

// struct IntegratorSinglePlane { nb_primitive, strategy } (src/integrators/explicit/plane_single.rs:280-294) + Integrator::compute, seed for seed the reference:
// the planes from the main sampler (rl_plane_generate), the plane tree (rl_plane_map_build), the block seeds from the sampler the generation leaves, the
// gather on reference-order streams (rl_render_plane_single).  generate = Lanes and tree_build = Device set the context options plane_generate_lanes and
// plane_tree_device, under which the two calls forward to rl_plane_generate_lanes (one lane per iteration) and rl_plane_map_build_device (the tree from
// device kernels): the same planes and the same map, byte for byte.
enum class PlaneGenerate { Serial, Lanes };
struct IntegratorSinglePlane {
    uint32_t nb_primitive = 128;
    rl_plane_strategy strategy = RL_PLANE_STRATEGY_AVERAGE;
    PlaneGenerate generate{PlaneGenerate::Serial};
    TreeBuild tree_build{TreeBuild::Host};
    int device = 0;
    Options options;
    rl_render_stats last_stats{}, last_generation_stats{};
    BufferCollection compute(IndependentSampler& sampler, Scene& scene) {
        RenderContext ctx(scene, device, options);
        if (generate == PlaneGenerate::Lanes) check(rl_context_set_option(ctx, "plane_generate_lanes", "1"), "plane-single");
        if (tree_build == TreeBuild::Device) check(rl_context_set_option(ctx, "plane_tree_device", "1"), "plane-single");
        return compute_with_map(ctx, sampler, scene, "plane-single",
            [&](rl_plane_set** out) { return rl_plane_generate(ctx, nb_primitive, strategy, &sampler.rnd, out, &last_generation_stats); }, rl_plane_destroy,
            [&](const rl_plane_set* planes, rl_plane_map** out) { return rl_plane_map_build(ctx, planes, out); }, rl_plane_map_destroy, rl_render_plane_single, &last_stats);
    }
};

// struct IntegratorSinglePlaneUncorrelated { nb_primitive, strategy } (src/integrators/explicit/uncorrelated_plane_single.rs:8-11) + Integrator::compute, seed for
// seed the reference: the block seeds straight from the main sampler (:83), then every camera sample makes and gathers its own planes (rl_render_plane_uncorrelated).
struct IntegratorSinglePlaneUncorrelated {
    uint32_t nb_primitive = 128;
    rl_plane_strategy strategy = RL_PLANE_STRATEGY_AVERAGE;
    int device = 0;
    Options options;
    rl_render_stats last_stats{};
    BufferCollection compute(IndependentSampler& sampler, Scene& scene) {
        RenderContext ctx(scene, device, options);
        const std::vector<uint64_t> seeds = ctx.block_seeds(sampler);
        check(rl_render_plane_uncorrelated(ctx, nb_primitive, strategy, (uint32_t)scene.nb_samples, sampler.variant, 0, 1, seeds.data(), seeds.size(), ctx.img.primal.data(), &last_stats),
              "plane-single --uncorrelated");
        return std::move(ctx.img);
    }
};

// compute of the four point-normal structs below: the block seeds straight from the main sampler, `self`'s fields into the params `defaults` fills, `render`
template <class Self, class Params, class Defaults>
BufferCollection compute_point_normal(Self& self, IndependentSampler& sampler, Scene& scene, Defaults&& defaults,
                                      int (*render)(rl_context*, const Params*, const uint64_t*, size_t, float*, rl_render_stats*), const char* what) {
    RenderContext ctx(scene, self.device, self.options);
    const std::vector<uint64_t> seeds = ctx.block_seeds(sampler);
    Params p;
    defaults(&p);
    p.spp = (uint32_t)scene.nb_samples; p.strategy = self.strategy; p.use_aa = self.use_aa ? 1 : 0; p.stream_mode = self.stream_mode; p.seed_variant = sampler.variant;
    check(render(ctx, &p, seeds.data(), seeds.size(), ctx.img.primal.data(), &self.last_stats), what);
    return std::move(ctx.img);
}

// struct IntegratorPointNormal { strategy, use_mis, warps, warps_strategy, splitting, use_aa } (src/integrators/explicit/point_normal.rs:1172-1179) +
// Integrator::compute -> compute_mc (:1181-1199), seed for seed the reference: the block seeds straight from the main sampler, then rl_render_point_normal.
// The seven plain strategies; the CLI refuses the flavoured ones, MIS, splitting and the warps before it gets here.
struct IntegratorPointNormal {
    rl_pn_strategy strategy = RL_PN_TR_EX;
    bool use_aa = true;
    rl_stream_mode stream_mode = RL_STREAM_REFERENCE_ORDER;
    int device = 0;
    Options options;
    rl_render_stats last_stats{};
    BufferCollection compute(IndependentSampler& sampler, Scene& scene) {
        return compute_point_normal(*this, sampler, scene, rl_point_normal_params_default, rl_render_point_normal, "point-normal");
    }
};

// IntegratorPointNormal with use_mis = true (point_normal.rs:2605-2612): compute_multiple_tr, compute_multiple_equiangular or compute_multiple_strategy by the
// strategy's distance family, through rl_render_point_normal_mis.  A struct of its own: IntegratorPointNormal above stays the seven plain estimators.
struct IntegratorPointNormalMis {
    rl_pn_strategy strategy = RL_PN_TR_EX;
    bool use_aa = true;
    rl_stream_mode stream_mode = RL_STREAM_REFERENCE_ORDER;
    int device = 0;
    Options options;
    rl_render_stats last_stats{};
    BufferCollection compute(IndependentSampler& sampler, Scene& scene) {
        return compute_point_normal(*this, sampler, scene, rl_point_normal_mis_params_default, rl_render_point_normal_mis, "point-normal-mis");
    }
};

// IntegratorPointNormal with one of its six Taylor strategies (point_normal.rs:1276-1290, 1404-1418): TaylorSampling or PointNormalTaylorSampling behind
// compute_single_strategy's EX arm, through rl_render_point_normal_taylor.  A struct of its own, as IntegratorPointNormalMis is.
struct IntegratorPointNormalTaylor {
    rl_pn_taylor_strategy strategy = RL_PN_TAYLOR_EQ_TR;
    bool use_aa = true;
    rl_stream_mode stream_mode = RL_STREAM_REFERENCE_ORDER;
    int device = 0;
    Options options;
    rl_render_stats last_stats{};
    BufferCollection compute(IndependentSampler& sampler, Scene& scene) {
        return compute_point_normal(*this, sampler, scene, rl_point_normal_taylor_params_default, rl_render_point_normal_taylor, "point-normal-taylor");
    }
};

// IntegratorPointNormal over the light tree (fix_random_sample_emitter's ATS arm, point_normal.rs:1217-1228, and compute_single_tr's, :2237-2243), through
// rl_render_point_normal_ats: `strategy` is an rl_pn_strategy (family plain) or an rl_pn_taylor_strategy (family Taylor).  The scene's emitters are built
// with the tree.
struct IntegratorPointNormalAts {
    rl_pn_ats_family family = RL_PN_ATS_PLAIN;
    int32_t strategy = RL_PN_EQ_EX;
    bool use_aa = true;
    rl_stream_mode stream_mode = RL_STREAM_REFERENCE_ORDER;
    int device = 0;
    Options options;
    rl_render_stats last_stats{};
    BufferCollection compute(IndependentSampler& sampler, Scene& scene) {
        // compute_point_normal fills the fields the four structs share; the family goes in behind the defaults
        const auto defaults = [&](rl_point_normal_ats_params* p) { rl_point_normal_ats_params_default(p); p->family = family; };
        return compute_point_normal(*this, sampler, scene, defaults, rl_render_point_normal_ats, "point-normal-ats");
    }
};

// IntegratorAverage (src/integrators/avg.rs:5-131) and IntegratorEqualTime (src/integrators/equal_time.rs:4-66):
// host loops around any inner integrator with `compute(IndependentSampler&, Scene&)`.
template <class T, class = void> struct has_frames_in_flight : std::false_type {};
template <class T> struct has_frames_in_flight<T, std::void_t<decltype(std::declval<T&>().frames_in_flight)>> : std::true_type {};
template <class Inner>
struct IntegratorAverage {
    Inner& integrator;
    std::optional<size_t> time_out;   // seconds
    bool dump_all = true;
    BufferCollection compute(IndependentSampler& sampler, Scene& scene) {
        if (!dump_all && !time_out) throw std::runtime_error("Impossible to have infinite approach and not dumping all images");
        const std::string& out = scene.output_img_path;
        size_t dot = out.rfind('.');
        if (dot == std::string::npos) throw std::runtime_error("No file extension provided");
        const std::string base = out.substr(0, dot), ext = out.substr(dot + 1);
        FILE* csv = dump_all ? std::fopen((base + "_time.csv").c_str(), "w") : nullptr;
        if (dump_all && !csv) throw std::runtime_error("cannot write " + base + "_time.csv");
        BufferCollection bitmap;
        size_t iteration = 1;
        double elapsed = 0.0;
        // frames in flight (an inner integrator with frames_in_flight > 1): the passes are rendered a batch at a time and folded in pass order, each charged its
        // share of the batch's time; the passes of the last batch beyond the time-out are dropped (their seeds are drawn)
        std::vector<BufferCollection> pending;
        size_t next_pending = 0;
        double share = 0.0;
        for (;;) {
            auto t0 = std::chrono::steady_clock::now();
            BufferCollection nb;
            if constexpr (has_frames_in_flight<Inner>::value) {
                if (integrator.frames_in_flight > 1) {
                    if (next_pending == pending.size()) {
                        pending = integrator.compute_frames(sampler, scene, (size_t)integrator.frames_in_flight);
                        next_pending = 0;
                        share = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / (double)pending.size();
                    }
                    nb = std::move(pending[next_pending++]);
                    elapsed += share;
                    t0 = std::chrono::steady_clock::now();
                } else nb = integrator.compute(sampler, scene);
            } else nb = integrator.compute(sampler, scene);
            if (iteration == 1) bitmap = nb;
            else { bitmap.scale((float)iteration); bitmap.accumulate_bitmap(nb); bitmap.scale(1.0f / (float)(iteration + 1)); }   // avg.rs:59-61
            elapsed += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (dump_all) {
                bitmap.save("primal", base + "_" + std::to_string(iteration) + "." + ext);
                std::fprintf(csv, "%llu.%u,\n", (unsigned long long)elapsed, (unsigned)((elapsed - (double)(unsigned long long)elapsed) * 1000.0));
            }
            if (time_out && (size_t)elapsed >= *time_out) break;
            iteration++;
        }
        if (csv) std::fclose(csv);
        return bitmap;
    }
};
template <class Inner>
struct IntegratorEqualTime {
    Inner& integrator;
    double target_time_ms;
    size_t iterations = 0;
    BufferCollection compute(IndependentSampler& sampler, Scene& scene) {
        BufferCollection bitmap;
        size_t iteration = 1;
        double elapsed_ms = 0.0;
        std::vector<BufferCollection> pending;      // frames in flight: as in IntegratorAverage
        size_t next_pending = 0;
        double share_ms = 0.0;
        for (;;) {
            auto t0 = std::chrono::steady_clock::now();
            BufferCollection nb;
            if constexpr (has_frames_in_flight<Inner>::value) {
                if (integrator.frames_in_flight > 1) {
                    if (next_pending == pending.size()) {
                        pending = integrator.compute_frames(sampler, scene, (size_t)integrator.frames_in_flight);
                        next_pending = 0;
                        share_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / (double)pending.size();
                    }
                    nb = std::move(pending[next_pending++]);
                    elapsed_ms += share_ms;
                    t0 = std::chrono::steady_clock::now();
                } else nb = integrator.compute(sampler, scene);
            } else nb = integrator.compute(sampler, scene);
            if (iteration == 1) bitmap = nb; else bitmap.accumulate_bitmap(nb);
            elapsed_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (elapsed_ms >= target_time_ms) break;
            iteration++;
        }
        bitmap.scale(1.0f / (float)iteration);
        iterations = iteration;
        return bitmap;
    }
};

}  // namespace rustlight
