// cli.cpp — `rustlight-amd`: the reference CLI's flags for the `path` subcommand (examples/cli.rs:
// global flags 106-145, `path` 162-169, medium 355-399, sampler 876-896, run/save 898-923).
//   rustlight-amd <scene.pbrt|scene.xml> -n SPP -o out.pfm [-r independent[:SEED]|stratified[:SEED]] [-m s[:a[:g]]] [-s SCALE] [-t N]
//                 [--device D] [--gpus N] [--frames-in-flight K] [--stream-mode reference|per-sample] [--numerics exact|fast] [--option name=value ...]
//                 path [-m MAX|inf] [-n MIN] [-r RR|inf] [-x] [-s all|bsdf|emitter]
//               | ao [-d DIST|inf] [-n]            (examples/cli.rs:149-154)
//               | direct [-b NB_BSDF] [-l NB_LIGHT] (examples/cli.rs:155-160)
//               | light-tracing [-m MAX|inf] [-n MIN] [-r RR|inf] [-s all|surface|volume]   (examples/cli.rs:54-61, 170-174; per-sample streams)
//               | vpl [-m MAX|inf] [-r RR|inf] [-b CLAMP] [--nb-vpl N] [-l all|surface|volume] [-v all|surface|volume] [--light-streams reference|per-path]   (examples/cli.rs:176-184, 707-733;
//                 -b is accepted and ignored as the reference ignores clamping_factor; -n is refused: the reference declares it twice under `vpl`)
//               | vol-primitivies [-m MAX|inf] [-n MIN] [-r RR|inf] [--nb-primitive N] [-p bre] [--radius R] [--light-streams reference|per-path] [--tree-build host|device]   (examples/cli.rs:189-196, 692-716; sic, `vol-primitives`
//                 is accepted too.  -p defaults to bre: the reference's default "BRE" matches none of its own arms and panics; beam | plane | vrl are not
//                 built.  -n is min_depth, parsed and ignored as the reference ignores it here — its short form of --nb-primitive clashes with it.  --radius: the
//                 photon radius, the reference's hard-coded 0.001 unless given)
//                 --light-streams (vpl, vol-primitivies): reference = the light paths on the main sampler's serial stream, seed for seed the reference (default);
//                 per-path = one light path per GPU lane, each on its own stream (rl_vpl_generate_paths): statistically, not seed-for-seed, the same image
//                 --tree-build (vol-primitivies): host = the photon tree built on the host (default); device = the same tree, byte for byte, built by device
//                 kernels with no record leaving the GPU (rl_photon_map_build_device)
//               | photon-beams [-m MAX|inf] [-n MIN] [-r RR|inf] [--nb-primitive N] [--radius R] [--light-streams reference|per-path]   (IntegratorVolPrimitives with
//                 primitives = Beams, vol_primitives.rs; a subcommand of its own: `vol-primitivies -p beam` stays refused with the other unbuilt primitives.  The
//                 options and limits of vol-primitivies; N is 1 .. RL_BEAM_MAX; no --tree-build: the split and the beam tree are built on the host)
//               | photon-planes [-m MAX|inf] [-n MIN] [-r RR|inf] [--nb-primitive N] [--radius R] [--light-streams reference|per-path]   (IntegratorVolPrimitives with
//                 primitives = Planes; a subcommand of its own as photon-beams is: `vol-primitivies -p plane` stays refused.  photon-beams' options and limits;
//                 MAX >= 4: no light path holds a plane below that; no --tree-build and no -p / -s)
//               | virtual-ray-lights [-m MAX|inf] [-n MIN] [-r RR|inf] [--nb-primitive N] [--radius R] [--light-streams reference|per-path]   (IntegratorVolPrimitives
//                 with primitives = VRL; a subcommand of its own as photon-beams is: `vol-primitivies -p vrl` stays refused.  photon-beams' options and limits: the
//                 beams are its beam pass's, the ones that leave a volume vertex are the VRLs)
//               | plane-single [-n|--nb-primitive N] [-s|--strategy uv|ut|vt|average|discrete_mis|ualpha|cmis]   (examples/cli.rs:197-202, 664-691; needs -m;
//                 the limits of vol-primitivies: independent sampler, reference-order streams, exact numerics, one device, one pass)
//                 --uncorrelated: IntegratorSinglePlaneUncorrelated (uncorrelated_plane_single.rs; the reference's subcommand `uncorrelated-plane-single`, cli.rs): every
//                 camera sample makes its own N planes; the same options, limits and refusals
//               | point-normal [-s|--strategy tr_ex|tr_phase|eq_ex|eq_phase|eq_clamped_ex|eq_clamped_phase|pn_ex] [-z|--disable-aa]   (examples/cli.rs:209-224,
//                 436-521; needs -m; both stream modes; independent sampler, exact numerics, one device, one pass, no light tree.  The flavoured strategies
//                 (Taylor, warp, best), -x / --use-mis, -k / --splitting, -w / --warps and --warps-strategy are not built and are refused by name)
//               | point-normal-mis [-s|--strategy NAME] [-z|--disable-aa]   (the reference's `point-normal -x`: IntegratorPointNormal with use_mis; NAME is one
//                 of point-normal's seven, of which only the distance family matters; the limits and refusals of point-normal; -x, -k, -w, --warps-strategy
//                 and the flavoured strategies are refused by name)
//               | point-normal-taylor [-s|--strategy eq_phase_taylor_ex|eq_tr_taylor_ex|eq_clamped_phase_taylor_ex|eq_clamped_tr_taylor_ex|pn_tr_taylor_ex|
//                 pn_phase_taylor_ex] [-z|--disable-aa]   (the reference's `point-normal -s <a Taylor name>`; default eq_tr_taylor_ex; the limits and refusals
//                 of point-normal; -x, -k, -w, --warps-strategy, the plain names and the warp / best names are refused by name)
//               | point-normal-ats [-s|--strategy NAME] [-z|--disable-aa]   (the reference's `-x ats point-normal`: the emitter from the light tree, walked
//                 with the ray importance; NAME is one of point-normal's seven or of point-normal-taylor's six, default eq_ex; the scene's emitters are built
//                 with the tree whether or not `-x ats` is given; the limits and refusals of point-normal-taylor; -x (MIS), -k, -w, --warps-strategy and the
//                 warp / best names are refused by name)
// Note `-n` / `-m` / `-r` / `-s` mean spp / medium / sampler / scale before the subcommand and
// min-depth / max-depth / rr-depth / strategy after it, exactly as in the reference.
//
// The layout: Args holds what the command line said, SUBCOMMANDS one record per subcommand — its name, whether it takes --light-streams and --tree-build,
// and three functions: `option` consumes one option after the subcommand, `check` refuses what the subcommand cannot do before a device is opened and
// leaves what it parsed in Args, `run` builds the integrator and renders.  main is the sequence: parse, check, sampler, scene, run, save.
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <sstream>
#include <type_traits>

#include "integrator.hpp"

using namespace rustlight;

// one line on stderr and the exit code: 2 for what the command line asks and cannot have, 1 for what the scene setup fails at
[[noreturn]] static void quit(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
static void quit(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(stderr, fmt, ap);
    va_end(ap);
    std::exit(code);
}

static std::optional<uint32_t> match_infinity(const std::string& s) {   // cli.rs:31-39
    if (s == "inf") return std::nullopt;
    char* e = nullptr;
    unsigned long v = std::strtoul(s.c_str(), &e, 10);
    if (!e || *e) quit(2, "wrong input for inf type parameter\n");
    return (uint32_t)v;
}

// --nb-vpl / --nb-primitive: 1 .. RL_VPL_MAX
static uint32_t parse_count(const char* flag, const std::string& s) {
    char* end = nullptr;
    const unsigned long long n = std::strtoull(s.c_str(), &end, 10);
    if (s.empty() || *end != '\0' || n == 0 || n > (unsigned long long)RL_VPL_MAX) quit(2, "invalid %s: %s (1 .. %d)\n", flag, s.c_str(), (int)RL_VPL_MAX);
    return (uint32_t)n;
}
static float parse_radius(const std::string& s) {
    char* end = nullptr;
    const float r = std::strtof(s.c_str(), &end);
    if (s.empty() || *end != '\0' || !(r > 0.0f) || r > 3.0e38f) quit(2, "invalid --radius: %s (a finite number > 0)\n", s.c_str());
    return r;
}
// how the light paths draw (the gather stays in reference order either way)
static LightStreams parse_light_streams(const std::string& s) {
    if (s != "reference" && s != "per-path") quit(2, "invalid --light-streams: %s (reference or per-path)\n", s.c_str());
    return s == "per-path" ? LightStreams::PerPath : LightStreams::Reference;
}
// a strategy or option name among `names`, which stand in the order of the enum's values: its index, or -1
template <size_t N>
static int find_name(const std::string& s, const char* const (&names)[N]) {
    for (size_t k = 0; k < N; k++) if (s == names[k]) return (int)k;
    return -1;
}
// -m sigma_s[:sigma_a[:g]] (cli.rs:355-399)
struct Medium { size_t n_parts = 0; float sigma_s = 0.0f, sigma_a = 0.0f, g = 0.0f; };
static Medium parse_medium(const std::string& s) {
    std::vector<std::string> parts;
    std::stringstream ss(s);
    for (std::string tok; std::getline(ss, tok, ':');) parts.push_back(tok);
    Medium m;
    m.n_parts = parts.size();
    if (parts.size() > 0) m.sigma_s = std::strtof(parts[0].c_str(), nullptr);
    if (parts.size() > 1) m.sigma_a = std::strtof(parts[1].c_str(), nullptr);
    if (parts.size() > 2) m.g = std::strtof(parts[2].c_str(), nullptr);
    return m;
}
static bool is_stratified(const std::string& rng) { return rng == "stratified" || rng.rfind("stratified:", 0) == 0; }

struct Subcommand;
struct Args {
    // before the subcommand
    std::string scene_path, output, medium = "0.0", rng = "independent", average, equal_time;
    size_t nbsamples = 1;
    float scale_image = 1.0f;
    int device = 0, gpus = 1, frames_in_flight = 1;
    bool use_ats = false, shading_normals = true;
    int light_override = RL_EMISSION_COLOR;             // -x hvs-light | texture-light
    rl_stream_mode mode = RL_STREAM_REFERENCE_ORDER;    // like rustlight; `--stream-mode per-sample` trades the seed-for-seed image for throughput
    bool mode_given = false;                            // (-r stratified sets the mode itself)
    uint32_t numerics = RL_NUMERICS_EXACT;
    Options options;
    // the subcommand and its options as they were given: each subcommand's `option` fills the ones it has
    const Subcommand* cmd = nullptr;
    std::string max_depth = "inf", min_depth = "0", rr_depth = "0";
    std::optional<std::string> strategy;                // -s: who reads it knows its default
    bool single_scattering = false;
    std::string ao_distance = "1.0";
    bool ao_normal_correction = false;
    size_t nb_bsdf = 1, nb_light = 1;
    std::string nb = "128";                             // --nb-vpl / --nb-primitive
    std::string option_lt = "all", option_vpl = "all";
    std::string primitives = "bre", radius = "0.001";
    std::string light_streams = "reference";            // `--light-streams per-path` shoots the light paths in parallel, each on its own stream
    std::string tree_build = "host";                    // `--tree-build device` builds the photon tree on the GPU
    bool uncorrelated = false;
    std::string unbuilt;                                // IntegratorPointNormal: the first option given that is not built
    bool disable_aa = false;
    // what the subcommand's `check` and the sampler parse made of them, for `run`
    std::optional<uint32_t> max, min, rr;
    int strategy_index = 0, lt_index = 0, vpl_index = 0;
    int family = 0;      // point-normal-ats: rl_pn_ats_family of the strategy's name
    uint32_t count = 0;
    float radius_value = 0.0f;
    LightStreams streams = LightStreams::Reference;
    TreeBuild tree = TreeBuild::Host;
    uint64_t seed = 0;
};

// the command line and the place in it; value(): the word after the option at that place, which the option consumes
struct Words {
    int argc;
    char** argv;
    int i = 1;
    std::string value() {
        if (i + 1 >= argc) quit(2, "missing value for %s\n", argv[i]);
        return argv[++i];
    }
};

struct Rendered {
    BufferCollection img;
    double render_ms = 0.0;
    std::string info;      // INFO lines that belong after the elapsed time
};
struct Subcommand {
    const char* name;
    const char* alias;      // or nullptr
    bool light_streams, tree_build;      // takes --light-streams / --tree-build
    bool (*option)(Args&, const std::string& a, Words&);      // consumes the option `a` after the subcommand; false: the subcommand has no such option
    void (*check)(Args&);      // everything that is refused before a device is opened
    Rendered (*run)(const Args&, IndependentSampler&, Scene&);
};

// ---- what the subcommands share

// -m / -r after a subcommand, and -n where it is the min depth
static bool option_depths(Args& s, const std::string& a, Words& w, bool with_min = true) {
    if (a == "-m" || a == "--max-depth") s.max_depth = w.value();
    else if (a == "-r" || a == "--rr-depth") s.rr_depth = w.value();
    else if (with_min && (a == "-n" || a == "--min-depth")) s.min_depth = w.value();
    else return false;
    return true;
}

static void check_nothing(Args&) {}

// A light-pass command runs on the independent sampler, one kind of streams (`streams`: per-sample for the light tracer, reference order for the gathers), exact
// numerics and one device, and all but the light tracer (`one_pass`) in one pass: what it cannot do is refused here, before a device is opened
static void refuse_limits(const Args& s, rl_stream_mode streams, bool one_pass) {
    const char* why = nullptr;
    if (is_stratified(s.rng)) why = "-r stratified is not supported (independent[:SEED] only)";
    else if (s.mode_given && s.mode != streams) why = streams == RL_STREAM_PER_SAMPLE ? "--stream-mode reference is not supported (light paths use per-sample streams)" : "--stream-mode per-sample is not supported (the gather uses reference-order streams)";
    else if (s.numerics == RL_NUMERICS_FAST) why = "--numerics fast is not supported";
    else if (s.gpus > 1) why = "--gpus > 1 is not supported";
    else if (one_pass && (!s.average.empty() || !s.equal_time.empty())) why = "-a / -e are not supported";
    else if (one_pass && s.frames_in_flight > 1) why = "--frames-in-flight is not supported";
    if (why) quit(2, "%s: %s\n", s.cmd->name, why);
}

// "Volume integrator need a volume (add -m )": the medium string as the scene setup parses it
static void refuse_no_medium(const Args& s) {
    const Medium m = parse_medium(s.medium);
    if (m.sigma_a + m.sigma_s == 0.0f) quit(2, "%s: the integrator needs a medium (add -m SIGMA_S[:SIGMA_A[:G]])\n", s.cmd->name);
}

template <class Integrator>
static Rendered render(Integrator& it, IndependentSampler& sampler, Scene& scene) {
    Rendered r;
    r.img = it.compute(sampler, scene);
    r.render_ms = it.last_stats.render_ms;
    return r;
}

// -e SECONDS (cli.rs:898-907) and -a SECONDS|inf (cli.rs:908-917) around `inner`, or `inner` alone
template <class Inner>
static Rendered render_progressive(const Args& s, Inner& inner, IndependentSampler& sampler, Scene& scene) {
    Rendered r;
    if (!s.equal_time.empty()) {
        IntegratorEqualTime<Inner> eq{inner, std::strtod(s.equal_time.c_str(), nullptr) * 1000.0};
        r.img = eq.compute(sampler, scene);
        std::fprintf(stderr, "INFO Number iter: %zu\nINFO Number spp: %zu\n", eq.iterations, eq.iterations * scene.nb_samples);
    } else if (!s.average.empty()) {
        IntegratorAverage<Inner> av{inner, std::nullopt, true};
        if (s.average != "inf") av.time_out = (size_t)std::strtoull(s.average.c_str(), nullptr, 10);
        r.img = av.compute(sampler, scene);
    } else r.img = inner.compute(sampler, scene);
    r.render_ms = inner.last_stats.render_ms;
    return r;
}

// the fields the integrators with a light pass and a gather have in common
template <class Integrator>
static void set_light_pass(Integrator& it, const Args& s) {
    it.max_depth = s.max;
    it.rr_depth = s.rr;
    it.light_streams = s.streams;
    it.device = s.device;
    it.options = s.options;
}

// ---- IntegratorPathTracing (cli.rs:162-169).  Its depths and its strategy are parsed once the scene is loaded, as they always were

static bool option_path(Args& s, const std::string& a, Words& w) {
    if (option_depths(s, a, w)) return true;
    if (a == "-x" || a == "--single-scattering") s.single_scattering = true;
    else if (a == "-s" || a == "--strategy") s.strategy = w.value();
    else return false;
    return true;
}

// --gpus N: where the shards ran, how the framebuffers were merged, kernel ms per device
static std::string describe_multi(rl_multi* multi, int gpus) {
    std::string out;
    std::vector<char> buf(1 << 16);
    if (rl_multi_describe(multi, buf.data(), buf.size()) == RL_OK) out = std::string("INFO Multi-GPU: ") + buf.data() + "\n";
    for (int g = 0; g < gpus; g++) {
        int dev = -1; rl_render_stats st{};
        if (rl_multi_shard_stats(multi, g, &dev, &st) != RL_OK) continue;
        std::snprintf(buf.data(), buf.size(), "INFO shard %d on device %d: kernel %.2f ms (chain pass %.2f ms), %llu camera samples\n", g, dev, st.ms_other + st.ms_prepass, st.ms_prepass, (unsigned long long)st.camera_samples);
        out += buf.data();
    }
    return out;
}

static Rendered run_path(const Args& s, IndependentSampler& sampler, Scene& scene) {
    static const char* const names[] = {"all", "bsdf", "emitter"};      // IntegratorPathTracingStrategies, by value
    IntegratorPathTracing it;
    it.min_depth = match_infinity(s.min_depth);
    it.max_depth = match_infinity(s.max_depth);
    it.rr_depth = match_infinity(s.rr_depth);
    const std::string strategy = s.strategy.value_or("all");
    const int which = find_name(strategy, names);
    if (which < 0) quit(2, "invalid strategy: %s\n", strategy.c_str());
    it.strategy = (IntegratorPathTracingStrategies)which;
    it.single_scattering = s.single_scattering;
    it.device = s.device;
    it.n_gpus = s.gpus;      // --gpus N: blocks dealt round-robin over N devices, one RCCL reduce of the framebuffers over xGMI
    it.stream_mode = s.mode;
    it.numerics = s.numerics;
    it.frames_in_flight = s.frames_in_flight;      // -a / -e: that many independent passes on the GPU at once (same images, more of the chip busy)
    it.options = s.options;
    Rendered r = render_progressive(s, it, sampler, scene);
    if (it.multi) r.info = describe_multi(it.multi, s.gpus);
    return r;
}

// ---- IntegratorAO (cli.rs:149-154) and IntegratorDirect (cli.rs:155-160): nothing to refuse, and -a / -e pass them by

static bool option_ao(Args& s, const std::string& a, Words& w) {
    if (a == "-d" || a == "--distance") s.ao_distance = w.value();
    else if (a == "-n" || a == "--normal-correction") s.ao_normal_correction = true;
    else return false;
    return true;
}
static bool option_direct(Args& s, const std::string& a, Words& w) {
    if (a == "-b" || a == "--nb-bsdf-samples") s.nb_bsdf = std::strtoull(w.value().c_str(), nullptr, 10);
    else if (a == "-l" || a == "--nb-light-samples") s.nb_light = std::strtoull(w.value().c_str(), nullptr, 10);
    else return false;
    return true;
}
template <class Integrator>      // what IntegratorMC holds for both, then the render
static Rendered render_mc(Integrator& it, const Args& s, IndependentSampler& sampler, Scene& scene) {
    it.device = s.device;
    it.stream_mode = s.mode;
    return render(it, sampler, scene);
}
static Rendered run_ao(const Args& s, IndependentSampler& sampler, Scene& scene) {
    IntegratorAO it;
    it.normal_correction = s.ao_normal_correction;
    if (s.ao_distance == "inf") it.max_distance = std::nullopt; else it.max_distance = std::strtof(s.ao_distance.c_str(), nullptr);
    return render_mc(it, s, sampler, scene);
}
static Rendered run_direct(const Args& s, IndependentSampler& sampler, Scene& scene) {
    IntegratorDirect it;
    it.nb_bsdf_samples = s.nb_bsdf;
    it.nb_light_samples = s.nb_light;
    return render_mc(it, s, sampler, scene);
}

// ---- IntegratorLightTracing (cli.rs:54-61, 170-174)

static bool option_light(Args& s, const std::string& a, Words& w) {
    if (option_depths(s, a, w)) return true;
    if (a == "-s" || a == "--strategy") s.strategy = w.value();
    else return false;
    return true;
}
static void check_light(Args& s) {
    static const char* const names[] = {"all", "surface", "volume"};      // rl_light_strategy, by value
    refuse_limits(s, RL_STREAM_PER_SAMPLE, false);
    const std::string strategy = s.strategy.value_or("all");
    if ((s.strategy_index = find_name(strategy, names)) < 0) quit(2, "invalid light-tracing strategy: %s (all, surface or volume)\n", strategy.c_str());
    s.max = match_infinity(s.max_depth);
    s.min = match_infinity(s.min_depth);
    s.rr = match_infinity(s.rr_depth);
}
static Rendered run_light(const Args& s, IndependentSampler& sampler, Scene& scene) {
    IntegratorLightTracing it;
    it.strategy = (rl_light_strategy)s.strategy_index;
    it.max_depth = s.max;
    it.min_depth = s.min;
    it.rr_depth = s.rr;
    it.device = s.device;
    it.options = s.options;
    return render_progressive(s, it, sampler, scene);
}

// ---- IntegratorVPL (cli.rs:176-184)

static bool option_vpl(Args& s, const std::string& a, Words& w) {
    if (option_depths(s, a, w, false)) return true;
    if (a == "-b" || a == "--clamping") (void)w.value();           // clamping_factor: never read by the reference
    else if (a == "--nb-vpl") s.nb = w.value();
    else if (a == "-l" || a == "--option-lt") s.option_lt = w.value();
    else if (a == "-v" || a == "--option-vpl") s.option_vpl = w.value();
    else if (a == "--light-streams") s.light_streams = w.value();
    else if (a == "-n") quit(2, "vpl: -n is ambiguous in the reference (min_depth and nb_vpl share it); use --nb-vpl N\n");
    else return false;
    return true;
}
static void check_vpl(Args& s) {
    static const char* const names[] = {"all", "surface", "volume"};      // rl_vpl_option, by value
    s.streams = parse_light_streams(s.light_streams);
    refuse_limits(s, RL_STREAM_REFERENCE_ORDER, true);
    if ((s.lt_index = find_name(s.option_lt, names)) < 0) quit(2, "invalid vpl -l option: %s (all, surface or volume)\n", s.option_lt.c_str());
    if ((s.vpl_index = find_name(s.option_vpl, names)) < 0) quit(2, "invalid vpl -v option: %s (all, surface or volume)\n", s.option_vpl.c_str());
    s.count = parse_count("--nb-vpl", s.nb);
    s.max = match_infinity(s.max_depth);
    s.rr = match_infinity(s.rr_depth);
}
static Rendered run_vpl(const Args& s, IndependentSampler& sampler, Scene& scene) {
    IntegratorVPL it;
    it.option_lt = (rl_vpl_option)s.lt_index;
    it.option_vpl = (rl_vpl_option)s.vpl_index;
    it.nb_vpl = s.count;
    set_light_pass(it, s);
    return render(it, sampler, scene);
}

// ---- the three beam-pass integrators (IntegratorVolPrimitives with primitives = Beams, Planes, VRL), which differ in the struct and in the depth below which
// the integrator has nothing to gather (MinMaxDepth: no light path holds a plane below 4); the limits of the beam radiance estimate, and the medium the
// reference panics without

static bool option_beam_pass(Args& s, const std::string& a, Words& w) {
    if (option_depths(s, a, w)) return true;      // -n: `_min_depth` (cli.rs:697), never read
    if (a == "--nb-primitive") s.nb = w.value();
    else if (a == "--radius") s.radius = w.value();
    else if (a == "--light-streams") s.light_streams = w.value();
    else return false;
    return true;
}
template <uint32_t MinMaxDepth>
static void check_beam_pass(Args& s) {
    s.streams = parse_light_streams(s.light_streams);
    refuse_limits(s, RL_STREAM_REFERENCE_ORDER, true);
    s.count = parse_count("--nb-primitive", s.nb);
    if (s.count > (uint32_t)RL_BEAM_MAX) quit(2, "invalid --nb-primitive: %s (1 .. %d)\n", s.nb.c_str(), (int)RL_BEAM_MAX);
    s.radius_value = parse_radius(s.radius);
    refuse_no_medium(s);
    s.max = match_infinity(s.max_depth);
    if (s.max.has_value() && *s.max < MinMaxDepth) quit(2, "%s: -m %s is too small (no light path holds a plane below a max depth of %u)\n", s.cmd->name, s.max_depth.c_str(), MinMaxDepth);
    s.rr = match_infinity(s.rr_depth);
}
template <class Integrator>
static Rendered run_beam_pass(const Args& s, IndependentSampler& sampler, Scene& scene) {
    Integrator it;
    it.nb_primitive = s.count;
    it.radius = s.radius_value;
    set_light_pass(it, s);
    return render(it, sampler, scene);
}

// ---- IntegratorVolPrimitives (cli.rs:189-196): the beam pass's options, -p and --tree-build.  The primitives that are not built are refused first

static bool option_vol_primitives(Args& s, const std::string& a, Words& w) {
    if (option_beam_pass(s, a, w)) return true;
    if (a == "-p" || a == "--primitives") s.primitives = w.value();
    else if (a == "--tree-build") s.tree_build = w.value();
    else return false;
    return true;
}
static void check_vol_primitives(Args& s) {
    s.streams = parse_light_streams(s.light_streams);
    if (s.primitives == "beam" || s.primitives == "plane" || s.primitives == "vrl") quit(2, "vol-primitivies: -p %s is not built (bre only)\n", s.primitives.c_str());
    if (s.primitives != "bre") quit(2, "%s is not a correct primitive (bre, beam, plane, vrl)\n", s.primitives.c_str());
    refuse_limits(s, RL_STREAM_REFERENCE_ORDER, true);
    s.count = parse_count("--nb-primitive", s.nb);
    s.radius_value = parse_radius(s.radius);
    s.max = match_infinity(s.max_depth);
    s.rr = match_infinity(s.rr_depth);
    if (s.tree_build != "host" && s.tree_build != "device") quit(2, "invalid --tree-build: %s (host or device)\n", s.tree_build.c_str());
    s.tree = s.tree_build == "device" ? TreeBuild::Device : TreeBuild::Host;
}
static Rendered run_vol_primitives(const Args& s, IndependentSampler& sampler, Scene& scene) {
    IntegratorVolPrimitives it;
    it.nb_primitive = s.count;
    it.radius = s.radius_value;
    it.tree_build = s.tree;
    set_light_pass(it, s);
    return render(it, sampler, scene);
}

// ---- IntegratorSinglePlane (cli.rs:197-202) and, under --uncorrelated, IntegratorSinglePlaneUncorrelated: the same options, limits and refusals

static bool option_plane(Args& s, const std::string& a, Words& w) {
    if (a == "-n" || a == "--nb-primitive") s.nb = w.value();
    else if (a == "-s" || a == "--strategy") s.strategy = w.value();
    else if (a == "--uncorrelated") s.uncorrelated = true;
    else return false;
    return true;
}
static void check_plane(Args& s) {
    static const char* const names[] = {"uv", "vt", "ut", "average", "discrete_mis", "ualpha", "cmis"};      // rl_plane_strategy, by value
    const std::string strategy = s.strategy.value_or("average");
    if ((s.strategy_index = find_name(strategy, names)) < 0) quit(2, "%s is not a correct strategy choice (uv, ut, vt, average, discrete_mis, valpha, cmis)\n", strategy.c_str());
    refuse_limits(s, RL_STREAM_REFERENCE_ORDER, true);
    s.count = parse_count("--nb-primitive", s.nb);
    refuse_no_medium(s);
}
static Rendered run_plane(const Args& s, IndependentSampler& sampler, Scene& scene) {
    auto go = [&](auto&& it) {
        it.nb_primitive = s.count;
        it.strategy = (rl_plane_strategy)s.strategy_index;
        it.device = s.device;
        it.options = s.options;
        return render(it, sampler, scene);
    };
    return s.uncorrelated ? go(IntegratorSinglePlaneUncorrelated{}) : go(IntegratorSinglePlane{});
}

// ---- IntegratorPointNormal (cli.rs:209-224) and IntegratorPointNormalMis, the reference's `-x`: the seven plain strategies on either kind of streams — of
// which the MIS estimators read the distance family —, IntegratorPointNormalTaylor, the six Taylor strategies, and IntegratorPointNormalAts, both sets of
// names over the light tree; everything else of the reference's subcommand is refused by name

static bool option_point_normal(Args& s, const std::string& a, Words& w) {
    if (a == "-s" || a == "--strategy") s.strategy = w.value();
    else if (a == "-z" || a == "--disable-aa") s.disable_aa = true;
    else if (a == "-x" || a == "--use-mis") { if (s.unbuilt.empty()) s.unbuilt = a; }
    else if (a == "-k" || a == "--splitting" || a == "-w" || a == "--warps" || a == "--warps-strategy") { (void)w.value(); if (s.unbuilt.empty()) s.unbuilt = a; }
    else return false;
    return true;
}
template <class Integrator>
static void check_point_normal(Args& s) {
    static const char* const names[] = {"tr_ex", "tr_phase", "eq_ex", "eq_phase", "eq_clamped_ex", "eq_clamped_phase", "pn_ex"};      // rl_pn_strategy, by value
    static const char* const flavoured[] = {"eq_best_ex", "eq_warp_ex", "eq_phase_taylor_ex", "eq_tr_taylor_ex", "eq_clamped_best_ex", "eq_clamped_warp_ex",
                                            "eq_clamped_phase_taylor_ex", "eq_clamped_tr_taylor_ex", "pn_tr_taylor_ex", "pn_phase_taylor_ex", "pn_warp_ex", "pn_best_ex"};
    const char* list = "tr_ex, tr_phase, eq_ex, eq_phase, eq_clamped_ex, eq_clamped_phase, pn_ex";
    const std::string strategy = s.strategy.value_or("tr_ex");
    if (find_name(strategy, flavoured) >= 0) quit(2, "%s: -s %s is not built (%s)\n", s.cmd->name, strategy.c_str(), list);
    if ((s.strategy_index = find_name(strategy, names)) < 0) quit(2, "invalid strategy: %s (%s)\n", strategy.c_str(), list);
    if (!s.unbuilt.empty() && !std::is_same_v<Integrator, IntegratorPointNormalMis>) quit(2, "point-normal: %s is not built (MIS, splitting and the warps are left out)\n", s.unbuilt.c_str());
    if (!s.unbuilt.empty()) quit(2, "point-normal-mis: %s is not built (the subcommand is `point-normal -x` itself; splitting and the warps are left out)\n", s.unbuilt.c_str());
    if (s.use_ats) quit(2, "%s: -x ats is not built (the light tree's emitter sampling is left out)\n", s.cmd->name);
    refuse_limits(s, s.mode, true);      // both stream modes: the one given passes
    refuse_no_medium(s);
}
// point-normal-taylor: the six Taylor names of cli.rs:455-492 and nothing else of the reference's -s
static void check_point_normal_taylor(Args& s) {
    static const char* const names[] = {"eq_phase_taylor_ex", "eq_tr_taylor_ex", "eq_clamped_phase_taylor_ex", "eq_clamped_tr_taylor_ex", "pn_tr_taylor_ex",
                                        "pn_phase_taylor_ex"};      // rl_pn_taylor_strategy, by value
    static const char* const others[] = {"tr_ex", "tr_phase", "eq_ex", "eq_phase", "eq_clamped_ex", "eq_clamped_phase", "pn_ex", "eq_best_ex", "eq_warp_ex",
                                         "eq_clamped_best_ex", "eq_clamped_warp_ex", "pn_warp_ex", "pn_best_ex"};
    const char* list = "eq_phase_taylor_ex, eq_tr_taylor_ex, eq_clamped_phase_taylor_ex, eq_clamped_tr_taylor_ex, pn_tr_taylor_ex, pn_phase_taylor_ex";
    const std::string strategy = s.strategy.value_or("eq_tr_taylor_ex");
    if (find_name(strategy, others) >= 0) quit(2, "%s: -s %s is not built (%s)\n", s.cmd->name, strategy.c_str(), list);
    if ((s.strategy_index = find_name(strategy, names)) < 0) quit(2, "invalid strategy: %s (%s)\n", strategy.c_str(), list);
    if (!s.unbuilt.empty()) quit(2, "point-normal-taylor: %s is not built (MIS, splitting and the warps are left out)\n", s.unbuilt.c_str());
    if (s.use_ats) quit(2, "%s: -x ats is not built (the light tree's emitter sampling is left out)\n", s.cmd->name);
    refuse_limits(s, s.mode, true);      // both stream modes: the one given passes
    refuse_no_medium(s);
    const Medium m = parse_medium(s.medium);
    if (s.strategy_index == RL_PN_TAYLOR_PN_PHASE && (m.n_parts < 3 || m.g == 0.0f))
        quit(2, "%s: -s pn_phase_taylor_ex needs a Henyey-Greenstein medium with g != 0 (-m SIGMA_S:SIGMA_A:G; the reference asserts g != 0.0, point_normal.rs:1414)\n", s.cmd->name);
}
// point-normal-ats: the seven plain names and the six Taylor names over the light tree; what point-normal-taylor refuses, under its own name
static void check_point_normal_ats(Args& s) {
    static const char* const plain[] = {"tr_ex", "tr_phase", "eq_ex", "eq_phase", "eq_clamped_ex", "eq_clamped_phase", "pn_ex"};      // rl_pn_strategy, by value
    static const char* const taylor[] = {"eq_phase_taylor_ex", "eq_tr_taylor_ex", "eq_clamped_phase_taylor_ex", "eq_clamped_tr_taylor_ex", "pn_tr_taylor_ex",
                                         "pn_phase_taylor_ex"};      // rl_pn_taylor_strategy, by value
    static const char* const others[] = {"eq_best_ex", "eq_warp_ex", "eq_clamped_best_ex", "eq_clamped_warp_ex", "pn_warp_ex", "pn_best_ex"};
    const char* list = "tr_ex, tr_phase, eq_ex, eq_phase, eq_clamped_ex, eq_clamped_phase, pn_ex, eq_phase_taylor_ex, eq_tr_taylor_ex, eq_clamped_phase_taylor_ex, "
                       "eq_clamped_tr_taylor_ex, pn_tr_taylor_ex, pn_phase_taylor_ex";
    const std::string strategy = s.strategy.value_or("eq_ex");
    if (find_name(strategy, others) >= 0) quit(2, "%s: -s %s is not built (%s)\n", s.cmd->name, strategy.c_str(), list);
    s.family = 0;
    if ((s.strategy_index = find_name(strategy, plain)) < 0) { s.family = 1; s.strategy_index = find_name(strategy, taylor); }
    if (s.strategy_index < 0) quit(2, "invalid strategy: %s (%s)\n", strategy.c_str(), list);
    if (!s.unbuilt.empty()) quit(2, "point-normal-ats: %s is not built (MIS, splitting and the warps are left out)\n", s.unbuilt.c_str());
    refuse_limits(s, s.mode, true);      // both stream modes: the one given passes
    refuse_no_medium(s);
    const Medium m = parse_medium(s.medium);
    if (s.family == 1 && s.strategy_index == RL_PN_TAYLOR_PN_PHASE && (m.n_parts < 3 || m.g == 0.0f))
        quit(2, "%s: -s pn_phase_taylor_ex needs a Henyey-Greenstein medium with g != 0 (-m SIGMA_S:SIGMA_A:G; the reference asserts g != 0.0, point_normal.rs:1414)\n", s.cmd->name);
    s.use_ats = true;      // the subcommand is the light tree's: `-x ats point-normal-ats` is the same line
}
template <class Integrator>
static Rendered run_point_normal(const Args& s, IndependentSampler& sampler, Scene& scene) {
    Integrator it;
    if constexpr (std::is_same_v<Integrator, IntegratorPointNormalAts>) it.family = (rl_pn_ats_family)s.family;
    it.strategy = (decltype(it.strategy))s.strategy_index;
    it.use_aa = !s.disable_aa;
    it.stream_mode = s.mode;
    it.device = s.device;
    it.options = s.options;
    return render(it, sampler, scene);
}

static const Subcommand SUBCOMMANDS[] = {
    // name, alias, --light-streams, --tree-build, option, check, run
    {"path", nullptr, false, false, option_path, check_nothing, run_path},
    {"ao", nullptr, false, false, option_ao, check_nothing, run_ao},
    {"direct", nullptr, false, false, option_direct, check_nothing, run_direct},
    {"light-tracing", nullptr, false, false, option_light, check_light, run_light},
    {"vpl", nullptr, true, false, option_vpl, check_vpl, run_vpl},
    {"vol-primitivies", "vol-primitives", true, true, option_vol_primitives, check_vol_primitives, run_vol_primitives},      // (sic)
    {"photon-beams", nullptr, true, false, option_beam_pass, check_beam_pass<0>, run_beam_pass<IntegratorPhotonBeams>},
    {"photon-planes", nullptr, true, false, option_beam_pass, check_beam_pass<4>, run_beam_pass<IntegratorPhotonPlanes>},
    {"virtual-ray-lights", nullptr, true, false, option_beam_pass, check_beam_pass<0>, run_beam_pass<IntegratorVirtualRayLights>},
    {"plane-single", nullptr, false, false, option_plane, check_plane, run_plane},
    {"point-normal", nullptr, false, false, option_point_normal, check_point_normal<IntegratorPointNormal>, run_point_normal<IntegratorPointNormal>},
    {"point-normal-mis", nullptr, false, false, option_point_normal, check_point_normal<IntegratorPointNormalMis>, run_point_normal<IntegratorPointNormalMis>},
    {"point-normal-taylor", nullptr, false, false, option_point_normal, check_point_normal_taylor, run_point_normal<IntegratorPointNormalTaylor>},
    {"point-normal-ats", nullptr, false, false, option_point_normal, check_point_normal_ats, run_point_normal<IntegratorPointNormalAts>},
};
static const Subcommand* find_subcommand(const std::string& a) {
    for (const Subcommand& c : SUBCOMMANDS) if (a == c.name || (c.alias && a == c.alias)) return &c;
    return nullptr;
}

// ---- the command line

// -x / --xtra-options: ExtraOptions (cli.rs:41-50): ats | no-shading are honoured
static void extra_option(Args& s, const std::string& o) {
    if (o == "ats") s.use_ats = true;
    else if (o == "no-shading") s.shading_normals = false;
    else if (o == "hvs-light") s.light_override = RL_EMISSION_HSV;               // ExtraOptions::HVSLight (cli.rs:327, 410-429)
    else if (o == "texture-light") s.light_override = RL_EMISSION_TEXTURE;       // ExtraOptions::TextureLight
    else quit(2, "extra option %s is not supported by this drop-in (ats, no-shading, hvs-light, texture-light)\n", o.c_str());
}

// an option before the subcommand; false: `a` is none
static bool global_option(Args& s, const std::string& a, Words& w) {
    if (a == "-n" || a == "--nbsamples") s.nbsamples = std::strtoull(w.value().c_str(), nullptr, 10);
    else if (a == "-o" || a == "--output") s.output = w.value();
    else if (a == "-r" || a == "--random-number-generator") s.rng = w.value();
    else if (a == "-m" || a == "--medium") s.medium = w.value();
    else if (a == "-s" || a == "--scale-image") s.scale_image = std::strtof(w.value().c_str(), nullptr);
    else if (a == "-t" || a == "--threads") (void)w.value();   // host threads are irrelevant on the GPU path
    else if (a == "--device") s.device = std::atoi(w.value().c_str());
    else if (a == "--gpus") s.gpus = std::atoi(w.value().c_str());
    else if (a == "--frames-in-flight") s.frames_in_flight = std::max(1, std::atoi(w.value().c_str()));
    else if (a == "--stream-mode") { s.mode = w.value() == "reference" ? RL_STREAM_REFERENCE_ORDER : RL_STREAM_PER_SAMPLE; s.mode_given = true; }
    else if (a == "--numerics") s.numerics = w.value() == "fast" ? RL_NUMERICS_FAST : RL_NUMERICS_EXACT;
    else if (a == "--option") {   // an execution option of the device context(s): name=value (rl_context_set_option; none changes an image)
        const std::string o = w.value();
        const size_t eq = o.find('=');
        s.options.emplace_back(o.substr(0, eq), eq == std::string::npos ? std::string("1") : o.substr(eq + 1));
    }
    else if (a == "-a" || a == "--average") s.average = w.value();
    else if (a == "-e" || a == "--equal-time") s.equal_time = w.value();
    else if (a == "-x" || a == "--xtra-options") extra_option(s, w.value());
    else if (a == "-l" || a == "--log") (void)w.value();   // log file: nothing is logged on this path
    else if (a == "--light-streams") quit(2, "--light-streams is an option of the vpl, vol-primitivies, photon-beams, photon-planes and virtual-ray-lights subcommands: give it after the subcommand\n");
    else if (a == "--tree-build") quit(2, "--tree-build is an option of the vol-primitivies subcommand: give it after the subcommand\n");
    else return false;
    return true;
}

// Every word in order: up to the subcommand the global options and the scene, after it the subcommand's own options
static void parse_command_line(Args& s, int argc, char** argv) {
    for (Words w{argc, argv}; w.i < argc; w.i++) {
        const std::string a = argv[w.i];
        if (!s.cmd) {
            if ((s.cmd = find_subcommand(a)) || global_option(s, a, w)) continue;
            if (a[0] == '-') quit(2, "unknown option %s\n", a.c_str());
            if (!s.scene_path.empty()) quit(2, "only the `path`, `ao`, `direct`, `light-tracing`, `vpl`, `vol-primitivies`, `photon-beams`, `photon-planes`, `virtual-ray-lights`, `plane-single`, `point-normal` and `point-normal-mis` subcommands are provided (got %s)\n", a.c_str());
            s.scene_path = a;
        }
        else if (a == "--light-streams" && !s.cmd->light_streams) quit(2, "%s: --light-streams is not supported (photon-beams, photon-planes, virtual-ray-lights, vpl and vol-primitivies only)\n", s.cmd->name);
        else if (a == "--tree-build" && !s.cmd->tree_build) quit(2, "%s: --tree-build is not supported (vol-primitivies only)\n", s.cmd->name);
        else if (!s.cmd->option(s, a, w)) quit(2, "unknown %s option %s\n", s.cmd->name, a.c_str());
    }
    if (s.scene_path.empty() || s.output.empty() || !s.cmd)
        quit(2, "usage: rustlight-amd <scene.pbrt|scene.xml> -n SPP -o out.pfm [-r independent[:SEED]|stratified[:SEED]] [-m s[:a[:g]]] path [-m max] [-n min] [-r rr] [-x] [-s all|bsdf|emitter]\n");
}

// the sampler (cli.rs:876-896): the master sampler that draws the block seeds is IndependentSampler(SEED) for both kinds — OS entropy without a seed, as
// IndependentSampler::default() / StratifiedSampler's random() are; `stratified:SEED` is this drop-in's reproducible form.  stratified =
// RL_STREAM_STRATIFIED: StratifiedSampler::create(spp, 4) on every pixel (include/rustlight_amd.h)
static void parse_sampler(Args& s) {
    auto parse_seed = [&](const char* t) -> bool {
        if (!*t || *t == '-' || *t == '+' || *t == ' ') return false;
        char* e = nullptr;
        errno = 0;
        const unsigned long long v = std::strtoull(t, &e, 10);
        if (errno == ERANGE || !e || *e) return false;
        s.seed = v;
        return true;
    };
    if (s.rng == "independent") s.seed = std::random_device{}();   // IndependentSampler::default(): OS entropy
    else if (s.rng.rfind("independent:", 0) == 0) s.seed = std::strtoull(s.rng.c_str() + 12, nullptr, 10);
    else if (is_stratified(s.rng)) {
        if (s.rng == "stratified") s.seed = std::random_device{}();
        else if (!parse_seed(s.rng.c_str() + 11)) quit(2, "stratified sampler: the seed must be an unsigned 64-bit integer (got %s)\n", s.rng.c_str() + 11);
        if (s.mode_given) quit(2, "-r stratified sets the stream mode itself: it cannot be combined with --stream-mode\n");
        if (s.numerics == RL_NUMERICS_FAST) quit(2, "-r stratified is not built with --numerics fast\n");
        s.mode = RL_STREAM_STRATIFIED;
        size_t power_of4 = 1;
        while (power_of4 < s.nbsamples) power_of4 *= 4;
        if (power_of4 != s.nbsamples) std::fprintf(stderr, "WARN %zu is not 4 multiple (increase count to %zu), the stratified sampler will be less efficient!\n", s.nbsamples, power_of4);
    }
    else quit(2, "Wrong sampler type provided %s (independent[:seed] or stratified[:seed])\n", s.rng.c_str());
}

// ---- the scene

// "Overide light is needed" (cli.rs:410-429): every light mesh becomes HSV { scale } / Texture { scale, butterfly.jpg }
static void override_lights(const Args& s, Scene& scene) {
    int bitmap = -1;
    if (s.light_override == RL_EMISSION_TEXTURE) {
        uint32_t bw = 0, bh = 0;
        if (rl_load_image("butterfly.jpg", &bw, &bh, nullptr, 0) != RL_OK) quit(1, "texture-light: cannot read butterfly.jpg from the working directory (Bitmap::read(\"butterfly.jpg\"), cli.rs:423): %s\n", rl_last_error());
        std::vector<float> px((size_t)3 * bw * bh);
        if (rl_load_image("butterfly.jpg", &bw, &bh, px.data(), px.size()) != RL_OK) quit(1, "texture-light: %s\n", rl_last_error());
        bitmap = rl_scene_add_bitmap(scene.handle, bw, bh, px.data());
        if (bitmap < 0) quit(1, "texture-light: %s\n", rl_last_error());      // (a negative return is an error code, not a bitmap id)
    }
    if (rl_scene_override_light_emission(scene.handle, s.light_override, bitmap) != RL_OK) quit(1, "-x %s: %s\n", s.light_override == RL_EMISSION_HSV ? "hvs-light" : "texture-light", rl_last_error());
}

static void setup_scene(const Args& s, Scene& scene) {
    scene.nb_samples = s.nbsamples;
    scene.output_img_path = s.output;
    const Medium m = parse_medium(s.medium);
    if (m.n_parts > 3) quit(2, "invalid medium_density\n");
    if (m.sigma_a + m.sigma_s != 0.0f) {
        float sa[3] = {m.sigma_a, m.sigma_a, m.sigma_a}, s3[3] = {m.sigma_s, m.sigma_s, m.sigma_s};
        if (rl_scene_set_medium(scene.handle, sa, s3, m.n_parts > 2 ? RL_PHASE_HG : RL_PHASE_ISOTROPIC, m.g) != RL_OK) quit(2, "invalid medium_density\n");
    }
    if (s.scale_image != 1.0f && rl_scene_scale_image(scene.handle, s.scale_image) != RL_OK) quit(2, "invalid image scale: %s\n", rl_last_error());
    if (s.light_override != RL_EMISSION_COLOR) override_lights(s, scene);
    scene.build_emitters(s.use_ats);      // scene.build_emitters(use_ats) (cli.rs:432)
}

int main(int argc, char** argv) {
    Args s;
    parse_command_line(s, argc, argv);
    s.cmd->check(s);
    parse_sampler(s);
    try {
        std::unique_ptr<Scene> scene(Scene::load(s.scene_path, s.shading_normals));
        setup_scene(s, *scene);
        IndependentSampler sampler(s.seed);
        const Rendered r = s.cmd->run(s, sampler, *scene);
        std::fprintf(stderr, "INFO Elapsed Integrator: %.0f ms\n%s", r.render_ms, r.info.c_str());
        std::fprintf(stderr, "INFO Save final image: %s\n", s.output.c_str());
        r.img.save("primal", s.output);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "ERROR %s\n", e.what());
        return 1;
    }
    return 0;
}
