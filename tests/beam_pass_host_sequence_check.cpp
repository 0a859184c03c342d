// beam_pass_host_sequence_check.cpp — tests/host_sequence_check.cpp's check for the three beam-pass integrators, IntegratorPhotonBeams, IntegratorVirtualRayLights
// and IntegratorPhotonPlanes (host/integrator.hpp), as a program of its own: the host sequence — context, options, beam or plane pass, map, block seeds,
// render — against stub rl_* functions, no device, no library.  The stubs are written once over the set and map types; they count creates and destroys per
// handle kind, advance the sampler by a known amount per call, and can be told to fail at the k-th ABI call.  Each compute() runs once clean and once with
// each call of its sequence failing in turn, in both stream modes; after each run the exception text is the stub's error under the integrator's prefix,
// creates equal destroys for every kind, and the sampler stands where the calls that ran left it.  Built with the host sanitizers by
// tests/test_beam_pass_host_sequence.py, which also turns a leak or a double free into a failure.
#include <cstdio>
#include <cstring>
#include <string>

#include "../rustlight_amd/csrc/host/integrator.hpp"

// ---- the stubs
struct rl_scene { int unused; };
struct rl_context { int unused; };
struct rl_beam_set { int unused; };
struct rl_beam_map { int unused; };
struct rl_vrl_map { int unused; };
struct rl_pplane_set { int unused; };
struct rl_pplane_map { int unused; };

namespace {
enum Kind { CONTEXT, BEAM_SET, BEAM_MAP, VRL_MAP, PPLANE_SET, PPLANE_MAP, N_KINDS };
const char* const kKindName[N_KINDS] = {"context", "beam set", "beam map", "VRL map", "photon-plane set", "photon-plane map"};
const uint32_t kWidth = 40, kHeight = 24;                                  // 3 x 2 blocks of 16 x 16
const uint64_t kGenerateDraws = 1000;                                      // what a beam or plane pass advances the sampler by; a block seed advances it by 1
const float kRadius = 0.125f;

int g_created[N_KINDS], g_destroyed[N_KINDS];
int g_calls = 0, g_fail_at = 0;                                            // fallible ABI calls so far; the one that fails (0: none)
std::string g_error, g_failed_call, g_trace;
uint64_t g_expected_draws = 0;
float g_radius_seen = 0.0f;
uint32_t g_nb_seen = 0, g_spp_seen = 0;

// every fallible stub starts here: false = this is the call that fails
bool enter(const char* name) {
    g_calls++;
    g_trace += std::string(name) + " ";
    if (g_calls != g_fail_at) return true;
    g_failed_call = name;
    g_error = "stub failure in " + std::string(name) + " (call " + std::to_string(g_calls) + ")";
    return false;
}
template <class T> int create(Kind kind, T** out) { *out = new T{0}; g_created[kind]++; return RL_OK; }
template <class T> void destroy(Kind kind, T* h) { if (h) { g_destroyed[kind]++; delete h; } }
// the three calls of a sequence that differ by the set and map types alone
template <class Set>
int generate(const char* name, Kind kind, rl_context* ctx, const rl_path_params* p, uint32_t nb, rl_sampler* sampler, Set** out, rl_render_stats* stats) {
    *out = nullptr;
    if (!ctx || !p || !stats || !enter(name)) return RL_ERR_HIP;
    g_nb_seen = nb;
    sampler->s[0] += kGenerateDraws;                                       // (like the library: only a generation that succeeds moves the sampler)
    g_expected_draws += kGenerateDraws;
    return create(kind, out);
}
template <class Set, class Map>
int map_build(const char* name, Kind kind, rl_context* ctx, const Set* set, float radius, Map** out) {
    *out = nullptr;
    g_radius_seen = radius;
    return ctx && set && enter(name) ? create(kind, out) : RL_ERR_HIP;
}
template <class Map>
int render(const char* name, rl_context* ctx, const Map* map, uint32_t spp, uint32_t shard_index, uint32_t shard_count, const uint64_t* seeds, size_t n_blocks, float* out_rgb,
           rl_render_stats* stats) {
    if (!ctx || !map || !enter(name)) return RL_ERR_HIP;
    if (n_blocks != 6 || !seeds || !out_rgb || !stats || shard_index != 0 || shard_count != 1) return RL_ERR_INVALID_ARGUMENT;
    g_spp_seen = spp;
    for (size_t i = 0; i < (size_t)3 * kWidth * kHeight; i++) out_rgb[i] += 1.0f;      // (a zeroed image becomes all ones)
    stats->camera_samples = 7;
    return RL_OK;
}
}  // namespace

extern "C" {
const char* rl_last_error(void) { return g_error.c_str(); }
void rl_scene_destroy(rl_scene*) {}
int rl_scene_image_size(const rl_scene*, uint32_t* w, uint32_t* h) { *w = kWidth; *h = kHeight; return RL_OK; }
void rl_sampler_seed(rl_sampler* s, uint64_t seed, int) { s->s[0] = seed; s->s[1] = s->s[2] = s->s[3] = 0; }
void rl_path_params_default(rl_path_params* p) { std::memset(p, 0, sizeof(*p)); }
size_t rl_block_count(uint32_t w, uint32_t h) { return (size_t)((w + 15) / 16) * ((h + 15) / 16); }
int rl_generate_block_seeds(rl_sampler* master, uint32_t, uint32_t, uint64_t* seeds, size_t n) {
    for (size_t i = 0; i < n; i++) seeds[i] = master->s[0]++;
    g_expected_draws += n;
    return RL_OK;
}
int rl_context_create(const rl_scene*, int, rl_context** out) { *out = nullptr; return enter("rl_context_create") ? create(CONTEXT, out) : RL_ERR_HIP; }
void rl_context_destroy(rl_context* c) { destroy(CONTEXT, c); }
int rl_context_set_option(rl_context* c, const char*, const char*) { return c && enter("rl_context_set_option") ? RL_OK : RL_ERR_INVALID_ARGUMENT; }
int rl_beam_generate(rl_context* ctx, const rl_path_params* p, uint32_t nb, rl_sampler* sampler, rl_beam_set** out, rl_render_stats* stats) {
    return generate("rl_beam_generate", BEAM_SET, ctx, p, nb, sampler, out, stats);
}
int rl_beam_generate_paths(rl_context* ctx, const rl_path_params* p, uint32_t nb, rl_sampler* sampler, rl_beam_set** out, rl_render_stats* stats) {
    return generate("rl_beam_generate_paths", BEAM_SET, ctx, p, nb, sampler, out, stats);
}
int rl_pplane_generate(rl_context* ctx, const rl_path_params* p, uint32_t nb, rl_sampler* sampler, rl_pplane_set** out, rl_render_stats* stats) {
    return generate("rl_pplane_generate", PPLANE_SET, ctx, p, nb, sampler, out, stats);
}
int rl_pplane_generate_paths(rl_context* ctx, const rl_path_params* p, uint32_t nb, rl_sampler* sampler, rl_pplane_set** out, rl_render_stats* stats) {
    return generate("rl_pplane_generate_paths", PPLANE_SET, ctx, p, nb, sampler, out, stats);
}
void rl_beam_destroy(rl_beam_set* s) { destroy(BEAM_SET, s); }
void rl_pplane_destroy(rl_pplane_set* s) { destroy(PPLANE_SET, s); }
int rl_beam_map_build(rl_context* ctx, const rl_beam_set* set, float radius, rl_beam_map** out) { return map_build("rl_beam_map_build", BEAM_MAP, ctx, set, radius, out); }
int rl_vrl_map_build(rl_context* ctx, const rl_beam_set* set, float radius, rl_vrl_map** out) { return map_build("rl_vrl_map_build", VRL_MAP, ctx, set, radius, out); }
int rl_pplane_map_build(rl_context* ctx, const rl_pplane_set* set, float radius, rl_pplane_map** out) { return map_build("rl_pplane_map_build", PPLANE_MAP, ctx, set, radius, out); }
void rl_beam_map_destroy(rl_beam_map* m) { destroy(BEAM_MAP, m); }
void rl_vrl_map_destroy(rl_vrl_map* m) { destroy(VRL_MAP, m); }
void rl_pplane_map_destroy(rl_pplane_map* m) { destroy(PPLANE_MAP, m); }
int rl_render_beams(rl_context* ctx, const rl_beam_map* map, uint32_t spp, int32_t, uint32_t shard_index, uint32_t shard_count, const uint64_t* seeds, size_t n_blocks, float* out_rgb,
                    rl_render_stats* stats) {
    return render("rl_render_beams", ctx, map, spp, shard_index, shard_count, seeds, n_blocks, out_rgb, stats);
}
int rl_render_vrl(rl_context* ctx, const rl_vrl_map* map, uint32_t spp, int32_t, uint32_t shard_index, uint32_t shard_count, const uint64_t* seeds, size_t n_blocks, float* out_rgb,
                  rl_render_stats* stats) {
    return render("rl_render_vrl", ctx, map, spp, shard_index, shard_count, seeds, n_blocks, out_rgb, stats);
}
int rl_render_photon_planes(rl_context* ctx, const rl_pplane_map* map, uint32_t spp, int32_t, uint32_t shard_index, uint32_t shard_count, const uint64_t* seeds, size_t n_blocks,
                            float* out_rgb, rl_render_stats* stats) {
    return render("rl_render_photon_planes", ctx, map, spp, shard_index, shard_count, seeds, n_blocks, out_rgb, stats);
}
}  // extern "C"

// ---- the check
namespace {
int g_failures = 0;
void expect(bool ok, const std::string& what) {
    if (!ok) { g_failures++; std::printf("FAILED %s\n", what.c_str()); }
}

// One compute() with call `fail_at` failing (0: none).  Returns the number of ABI calls the run made.
template <class Integrator>
int run_once(const std::string& name, const std::string& prefix, int fail_at, Integrator& integrator) {
    std::memset(g_created, 0, sizeof g_created);
    std::memset(g_destroyed, 0, sizeof g_destroyed);
    g_calls = 0; g_fail_at = fail_at; g_expected_draws = 0;
    g_radius_seen = 0.0f; g_nb_seen = g_spp_seen = 0;
    g_error.clear(); g_failed_call.clear(); g_trace.clear();
    const std::string what = name + (fail_at ? ", call " + std::to_string(fail_at) + " failing" : ", clean");
    rl_scene scene_handle{0};
    rustlight::Scene scene(&scene_handle);
    scene.nb_samples = 2;
    const uint64_t seed = 5;
    rustlight::IndependentSampler sampler(seed);
    std::string thrown;
    bool threw = false;
    try {
        const rustlight::BufferCollection img = integrator.compute(sampler, scene);
        expect(img.width == kWidth && img.height == kHeight && img.primal.size() == (size_t)3 * kWidth * kHeight, what + ": the image has the scene's size");
        bool ones = true;
        for (float v : img.primal) ones = ones && v == 1.0f;
        expect(ones, what + ": the render wrote into the zeroed image that came back");
        expect(g_radius_seen == kRadius && g_nb_seen == integrator.nb_primitive && g_spp_seen == 2, what + ": radius, nb_primitive and spp reach the calls");
    } catch (const std::exception& e) { threw = true; thrown = e.what(); }
    expect(threw == (fail_at != 0), what + ": throws exactly when a call fails (" + thrown + ")");
    if (threw) {
        const std::string lead = g_failed_call == "rl_context_create" ? "rl_context_create: " : g_failed_call == "rl_context_set_option" ? "--option spec_force: " : prefix + ": ";
        expect(thrown == lead + g_error, what + ": the exception is `" + thrown + "`, not `" + lead + g_error + "`");
        expect(g_calls == fail_at, what + ": nothing is called after the failure (" + g_trace + ")");
    }
    for (int k = 0; k < N_KINDS; k++)
        expect(g_created[k] == g_destroyed[k], what + ": " + std::to_string(g_created[k]) + " " + kKindName[k] + " created, " + std::to_string(g_destroyed[k]) + " destroyed");
    expect(g_created[CONTEXT] == (fail_at == 1 ? 0 : 1), what + ": one context");
    expect(sampler.rnd.s[0] == seed + g_expected_draws, what + ": the sampler advanced by " + std::to_string(sampler.rnd.s[0] - seed) + ", the calls that ran by " + std::to_string(g_expected_draws));
    if (!fail_at) expect(g_expected_draws == kGenerateDraws + 6, what + ": the pass drew, then the block seeds");
    return g_calls;
}
// Both stream modes of one integrator: `pass` is its generation call's name, `tail` the calls that follow it
template <class Integrator>
void run_all(const std::string& struct_name, const std::string& prefix, const std::string& pass, const std::string& tail) {
    using namespace rustlight;
    for (LightStreams streams : {LightStreams::Reference, LightStreams::PerPath}) {
        const bool per_path = streams == LightStreams::PerPath;
        const std::string name = struct_name + (per_path ? " (per-path)" : "");
        Integrator integrator;
        integrator.nb_primitive = 77; integrator.radius = kRadius; integrator.light_streams = streams;
        integrator.options = {{"spec_force", "1"}};
        const int n = run_once(name, prefix, 0, integrator);
        const std::string want = "rl_context_create rl_context_set_option " + pass + (per_path ? "_paths " : " ") + tail + " ";
        expect(g_trace == want, name + ": the calls are `" + g_trace + "`, not `" + want + "`");
        expect(integrator.last_stats.camera_samples == 7, name + ": last_stats");
        for (int k = 1; k <= n; k++) run_once(name, prefix, k, integrator);
    }
}
}  // namespace

int main() {
    using namespace rustlight;
    run_all<IntegratorPhotonBeams>("IntegratorPhotonBeams", "photon-beams", "rl_beam_generate", "rl_beam_map_build rl_render_beams");
    run_all<IntegratorVirtualRayLights>("IntegratorVirtualRayLights", "virtual-ray-lights", "rl_beam_generate", "rl_vrl_map_build rl_render_vrl");
    run_all<IntegratorPhotonPlanes>("IntegratorPhotonPlanes", "photon-planes", "rl_pplane_generate", "rl_pplane_map_build rl_render_photon_planes");
    if (g_failures) { std::printf("%d checks failed\n", g_failures); return 1; }
    std::printf("beam-pass host sequence: OK\n");
    return 0;
}
