// host_sequence_check.cpp — a stand-alone check of the host sequence of IntegratorVPL, IntegratorVolPrimitives (both tree builds) and IntegratorSinglePlane
// (host/integrator.hpp) against stub rl_* functions: no device, no library.  The stubs count creates and destroys per handle kind, advance the sampler by a
// known amount per call, and can be told to fail at the k-th ABI call.  Every compute() runs once clean and once with each call of its sequence failing in
// turn; after each run the exception text is the stub's error under the integrator's prefix, creates equal destroys for every kind, and the sampler stands
// where the calls that ran left it.  Built with the host sanitizers by tests/test_host_sequence.py, which also turns a leak or a double free into a failure.
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>

#include "../rustlight_amd/csrc/host/integrator.hpp"

// ---- the stubs
struct rl_scene { int unused; };
struct rl_context { int unused; };
struct rl_vpl_set { int unused; };
struct rl_photon_map { int unused; };
struct rl_plane_set { int unused; };
struct rl_plane_map { int unused; };

namespace {
enum Kind { CONTEXT, VPL_SET, PHOTON_MAP, PLANE_SET, PLANE_MAP, N_KINDS };
const char* const kKindName[N_KINDS] = {"context", "vpl set", "photon map", "plane set", "plane map"};
const uint32_t kWidth = 40, kHeight = 24;                                  // 3 x 2 blocks of 16 x 16
const uint64_t kGenerateDraws = 1000, kPlaneDraws = 700;                   // what a generation advances the sampler by; a block seed advances it by 1

int g_created[N_KINDS], g_destroyed[N_KINDS];
int g_calls = 0, g_fail_at = 0;                                            // fallible ABI calls so far; the one that fails (0: none)
std::string g_error, g_failed_call, g_trace;
uint64_t g_expected_draws = 0;

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
int render(float* out_rgb, size_t n_blocks, rl_render_stats* stats) {
    if (n_blocks != 6 || !out_rgb || !stats) return RL_ERR_INVALID_ARGUMENT;
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
static int generate(const char* name, rl_context* ctx, rl_sampler* sampler, rl_vpl_set** out, rl_render_stats* stats) {
    *out = nullptr;
    if (!ctx || !stats || !enter(name)) return RL_ERR_HIP;
    sampler->s[0] += kGenerateDraws;                                       // (like the library: only a generation that succeeds moves the sampler)
    g_expected_draws += kGenerateDraws;
    return create(VPL_SET, out);
}
int rl_vpl_generate(rl_context* ctx, const rl_path_params*, uint32_t, int, rl_sampler* sampler, rl_vpl_set** out, rl_render_stats* stats) {
    return generate("rl_vpl_generate", ctx, sampler, out, stats);
}
int rl_vpl_generate_paths(rl_context* ctx, const rl_path_params*, uint32_t, int, rl_sampler* sampler, rl_vpl_set** out, rl_render_stats* stats) {
    return generate("rl_vpl_generate_paths", ctx, sampler, out, stats);
}
void rl_vpl_destroy(rl_vpl_set* s) { destroy(VPL_SET, s); }
int rl_render_vpl(rl_context* ctx, const rl_vpl_set* set, const rl_path_params*, int, const uint64_t*, size_t n_blocks, float* out_rgb, int, void*, rl_render_stats* stats) {
    return ctx && set && enter("rl_render_vpl") ? render(out_rgb, n_blocks, stats) : RL_ERR_HIP;
}
int rl_photon_map_build(rl_context* ctx, const rl_vpl_set* set, float, rl_photon_map** out) {
    *out = nullptr;
    return ctx && set && enter("rl_photon_map_build") ? create(PHOTON_MAP, out) : RL_ERR_HIP;
}
int rl_photon_map_build_device(rl_context* ctx, const rl_vpl_set* set, float, rl_photon_map** out, float*) {
    *out = nullptr;
    return ctx && set && enter("rl_photon_map_build_device") ? create(PHOTON_MAP, out) : RL_ERR_HIP;
}
void rl_photon_map_destroy(rl_photon_map* m) { destroy(PHOTON_MAP, m); }
int rl_render_bre(rl_context* ctx, const rl_photon_map* map, uint32_t, int32_t, uint32_t, uint32_t, const uint64_t*, size_t n_blocks, float* out_rgb, rl_render_stats* stats) {
    return ctx && map && enter("rl_render_bre") ? render(out_rgb, n_blocks, stats) : RL_ERR_HIP;
}
int rl_plane_generate(rl_context* ctx, uint32_t, int, rl_sampler* sampler, rl_plane_set** out, rl_render_stats* stats) {
    *out = nullptr;
    if (!ctx || !stats || !enter("rl_plane_generate")) return RL_ERR_HIP;
    sampler->s[0] += kPlaneDraws;
    g_expected_draws += kPlaneDraws;
    return create(PLANE_SET, out);
}
void rl_plane_destroy(rl_plane_set* s) { destroy(PLANE_SET, s); }
int rl_plane_map_build(rl_context* ctx, const rl_plane_set* set, rl_plane_map** out) {
    *out = nullptr;
    return ctx && set && enter("rl_plane_map_build") ? create(PLANE_MAP, out) : RL_ERR_HIP;
}
void rl_plane_map_destroy(rl_plane_map* m) { destroy(PLANE_MAP, m); }
int rl_render_plane_single(rl_context* ctx, const rl_plane_map* map, uint32_t, int32_t, uint32_t, uint32_t, const uint64_t*, size_t n_blocks, float* out_rgb, rl_render_stats* stats) {
    return ctx && map && enter("rl_render_plane_single") ? render(out_rgb, n_blocks, stats) : RL_ERR_HIP;
}
}  // extern "C"

// ---- the check
namespace {
int g_failures = 0;
void expect(bool ok, const std::string& what) {
    if (!ok) { g_failures++; std::printf("FAILED %s\n", what.c_str()); }
}

// One compute() with call `fail_at` failing (0: none).  Returns the number of ABI calls the run made.
int run_once(const std::string& name, const char* prefix, int fail_at, const std::function<rustlight::BufferCollection(rustlight::IndependentSampler&, rustlight::Scene&)>& compute) {
    std::memset(g_created, 0, sizeof g_created);
    std::memset(g_destroyed, 0, sizeof g_destroyed);
    g_calls = 0; g_fail_at = fail_at; g_expected_draws = 0;
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
        const rustlight::BufferCollection img = compute(sampler, scene);
        expect(img.width == kWidth && img.height == kHeight && img.primal.size() == (size_t)3 * kWidth * kHeight, what + ": the image has the scene's size");
        bool ones = true;
        for (float v : img.primal) ones = ones && v == 1.0f;
        expect(ones, what + ": the render wrote into the zeroed image that came back");
    } catch (const std::exception& e) { threw = true; thrown = e.what(); }
    expect(threw == (fail_at != 0), what + ": throws exactly when a call fails (" + thrown + ")");
    if (threw) {
        const std::string lead = g_failed_call == "rl_context_create" ? "rl_context_create: " : g_failed_call == "rl_context_set_option" ? "--option spec_force: " : prefix;
        expect(thrown == lead + g_error, what + ": the exception is `" + thrown + "`, not `" + lead + g_error + "`");
        expect(g_calls == fail_at, what + ": nothing is called after the failure (" + g_trace + ")");
    }
    for (int k = 0; k < N_KINDS; k++)
        expect(g_created[k] == g_destroyed[k], what + ": " + std::to_string(g_created[k]) + " " + kKindName[k] + " created, " + std::to_string(g_destroyed[k]) + " destroyed");
    expect(g_created[CONTEXT] == (fail_at == 1 ? 0 : 1), what + ": one context");
    expect(sampler.rnd.s[0] == seed + g_expected_draws, what + ": the sampler advanced by " + std::to_string(sampler.rnd.s[0] - seed) + ", the calls that ran by " + std::to_string(g_expected_draws));
    if (!fail_at) expect(g_expected_draws > 6, what + ": generation and block seeds both drew");
    return g_calls;
}
void run_all(const std::string& name, const char* prefix, int expected_calls, const std::function<rustlight::BufferCollection(rustlight::IndependentSampler&, rustlight::Scene&)>& compute) {
    const int n = run_once(name, prefix, 0, compute);
    expect(n == expected_calls, name + ": " + std::to_string(n) + " ABI calls (" + g_trace + "), expected " + std::to_string(expected_calls));
    for (int k = 1; k <= n; k++) run_once(name, prefix, k, compute);
}
}  // namespace

int main() {
    using namespace rustlight;
    const std::vector<std::pair<std::string, std::string>> options = {{"spec_force", "1"}};
    for (LightStreams streams : {LightStreams::Reference, LightStreams::PerPath}) {
        const std::string tag = streams == LightStreams::PerPath ? " (per-path)" : "";
        IntegratorVPL vpl;
        vpl.light_streams = streams; vpl.options = options;
        run_all("IntegratorVPL" + tag, "vpl: ", 4, [&](IndependentSampler& s, Scene& sc) { return vpl.compute(s, sc); });
        expect(vpl.last_stats.camera_samples == 7, "IntegratorVPL" + tag + ": last_stats");
        for (TreeBuild build : {TreeBuild::Host, TreeBuild::Device}) {
            IntegratorVolPrimitives volp;
            volp.light_streams = streams; volp.tree_build = build; volp.options = options;
            run_all("IntegratorVolPrimitives" + tag + (build == TreeBuild::Device ? " device tree" : " host tree"), "vol-primitives: ", 5,
                    [&](IndependentSampler& s, Scene& sc) { return volp.compute(s, sc); });
        }
    }
    IntegratorSinglePlane plane;
    plane.options = options;
    run_all("IntegratorSinglePlane", "plane-single: ", 5, [&](IndependentSampler& s, Scene& sc) { return plane.compute(s, sc); });
    if (g_failures) { std::printf("%d checks failed\n", g_failures); return 1; }
    std::printf("host sequence: OK\n");
    return 0;
}
