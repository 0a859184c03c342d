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
// Note `-n` / `-m` / `-r` / `-s` mean spp / medium / sampler / scale before the subcommand and
// min-depth / max-depth / rr-depth / strategy after it, exactly as in the reference.
#include <chrono>
#include <cstdio>
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <sstream>

#include "integrator.hpp"

using namespace rustlight;

static std::optional<uint32_t> match_infinity(const std::string& s) {   // cli.rs:31-39
    if (s == "inf") return std::nullopt;
    char* e = nullptr;
    unsigned long v = std::strtoul(s.c_str(), &e, 10);
    if (!e || *e) { std::fprintf(stderr, "wrong input for inf type parameter\n"); std::exit(2); }
    return (uint32_t)v;
}

// --nb-vpl / --nb-primitive: 1 .. RL_VPL_MAX
static bool parse_count(const char* flag, const std::string& s, uint32_t* out) {
    char* end = nullptr;
    const unsigned long long n = std::strtoull(s.c_str(), &end, 10);
    if (s.empty() || *end != '\0' || n == 0 || n > (unsigned long long)RL_VPL_MAX) { std::fprintf(stderr, "invalid %s: %s (1 .. %d)\n", flag, s.c_str(), (int)RL_VPL_MAX); return false; }
    *out = (uint32_t)n;
    return true;
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

int main(int argc, char** argv) {
    std::string scene_path, output, medium = "0.0", rng = "independent", strategy = "all";
    std::string max_depth = "inf", min_depth = "0", rr_depth = "0";
    size_t nbsamples = 1;
    float scale_image = 1.0f;
    int device = 0, gpus = 1;
    bool single_scattering = false, have_cmd = false, use_ats = false, shading_normals = true;
    int light_override = RL_EMISSION_COLOR;      // -x hvs-light | texture-light
    std::string cmd, ao_distance = "1.0", average, equal_time;
    bool ao_normal_correction = false;
    size_t nb_bsdf = 1, nb_light = 1;
    rl_stream_mode mode = RL_STREAM_REFERENCE_ORDER;   // like rustlight; `--stream-mode per-sample` trades the seed-for-seed image for throughput
    bool mode_given = false;                            // (-r stratified sets the mode itself)
    uint32_t numerics = RL_NUMERICS_EXACT;
    int frames_in_flight = 1;
    Options options;
    std::string nb_vpl = "128", option_lt = "all", option_vpl = "all";     // vpl (cli.rs:176-184)
    std::string nb_primitive = "128", primitives = "bre", radius = "0.001";     // vol-primitivies (cli.rs:189-196)
    std::string light_streams = "reference";            // vpl, vol-primitivies: `--light-streams per-path` shoots the light paths in parallel, each on its own stream
    std::string tree_build = "host";                    // vol-primitivies: `--tree-build device` builds the photon tree on the GPU
    std::string plane_nb = "128", plane_strategy = "average";     // plane-single (cli.rs:197-202)
    bool plane_uncorrelated = false;                              // plane-single --uncorrelated
    std::string pn_strategy = "tr_ex", pn_unbuilt;                // point-normal (cli.rs:209-224); pn_unbuilt: the first option given that is not built
    bool pn_disable_aa = false;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", a.c_str()); std::exit(2); } return argv[++i]; };
        if (!have_cmd) {
            if (a == "path" || a == "ao" || a == "direct" || a == "light-tracing" || a == "vpl") { have_cmd = true; cmd = a; }
            else if (a == "vol-primitivies" || a == "vol-primitives") { have_cmd = true; cmd = "vol-primitivies"; }
            else if (a == "plane-single" || a == "photon-beams" || a == "photon-planes" || a == "virtual-ray-lights" || a == "point-normal" || a == "point-normal-mis") { have_cmd = true; cmd = a; }
            else if (a == "-n" || a == "--nbsamples") nbsamples = std::strtoull(val().c_str(), nullptr, 10);
            else if (a == "-o" || a == "--output") output = val();
            else if (a == "-r" || a == "--random-number-generator") rng = val();
            else if (a == "-m" || a == "--medium") medium = val();
            else if (a == "-s" || a == "--scale-image") scale_image = std::strtof(val().c_str(), nullptr);
            else if (a == "-t" || a == "--threads") (void)val();   // host threads are irrelevant on the GPU path
            else if (a == "--device") device = std::atoi(val().c_str());
            else if (a == "--gpus") gpus = std::atoi(val().c_str());
            else if (a == "--frames-in-flight") frames_in_flight = std::max(1, std::atoi(val().c_str()));   // -a / -e: that many independent passes on the GPU at once (same images, more of the chip busy)
            else if (a == "--stream-mode") { mode = val() == "reference" ? RL_STREAM_REFERENCE_ORDER : RL_STREAM_PER_SAMPLE; mode_given = true; }
            else if (a == "--numerics") numerics = val() == "fast" ? RL_NUMERICS_FAST : RL_NUMERICS_EXACT;
            else if (a == "--option") {   // an execution option of the device context(s): name=value (rl_context_set_option; none changes an image)
                const std::string o = val();
                const size_t eq = o.find('=');
                options.emplace_back(o.substr(0, eq), eq == std::string::npos ? std::string("1") : o.substr(eq + 1));
            }
            else if (a == "-a" || a == "--average") average = val();
            else if (a == "-e" || a == "--equal-time") equal_time = val();
            else if (a == "-x" || a == "--xtra-options") {   // ExtraOptions (cli.rs:41-50): ats | no-shading are honoured
                const std::string o = val();
                if (o == "ats") use_ats = true;
                else if (o == "no-shading") shading_normals = false;
                else if (o == "hvs-light") light_override = RL_EMISSION_HSV;               // ExtraOptions::HVSLight (cli.rs:327, 410-429)
                else if (o == "texture-light") light_override = RL_EMISSION_TEXTURE;       // ExtraOptions::TextureLight
                else { std::fprintf(stderr, "extra option %s is not supported by this drop-in (ats, no-shading, hvs-light, texture-light)\n", o.c_str()); return 2; }
            }
            else if (a == "-l" || a == "--log") (void)val();   // log file: nothing is logged on this path
            else if (a == "--light-streams") { std::fprintf(stderr, "--light-streams is an option of the vpl, vol-primitivies, photon-beams, photon-planes and virtual-ray-lights subcommands: give it after the subcommand\n"); return 2; }
            else if (a == "--tree-build") { std::fprintf(stderr, "--tree-build is an option of the vol-primitivies subcommand: give it after the subcommand\n"); return 2; }
            else if (a[0] == '-') { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
            else if (scene_path.empty()) scene_path = a;
            else { std::fprintf(stderr, "only the `path`, `ao`, `direct`, `light-tracing`, `vpl`, `vol-primitivies`, `photon-beams`, `photon-planes`, `virtual-ray-lights`, `plane-single`, `point-normal` and `point-normal-mis` subcommands are provided (got %s)\n", a.c_str()); return 2; }
        } else if (a == "--light-streams" && cmd != "vpl" && cmd != "vol-primitivies" && cmd != "photon-beams" && cmd != "photon-planes" && cmd != "virtual-ray-lights") {
            std::fprintf(stderr, "%s: --light-streams is not supported (photon-beams, photon-planes, virtual-ray-lights, vpl and vol-primitivies only)\n", cmd.c_str()); return 2;
        } else if (a == "--tree-build" && cmd != "vol-primitivies") {
            std::fprintf(stderr, "%s: --tree-build is not supported (vol-primitivies only)\n", cmd.c_str()); return 2;
        } else if (cmd == "ao") {
            if (a == "-d" || a == "--distance") ao_distance = val();
            else if (a == "-n" || a == "--normal-correction") ao_normal_correction = true;
            else { std::fprintf(stderr, "unknown ao option %s\n", a.c_str()); return 2; }
        } else if (cmd == "direct") {
            if (a == "-b" || a == "--nb-bsdf-samples") nb_bsdf = std::strtoull(val().c_str(), nullptr, 10);
            else if (a == "-l" || a == "--nb-light-samples") nb_light = std::strtoull(val().c_str(), nullptr, 10);
            else { std::fprintf(stderr, "unknown direct option %s\n", a.c_str()); return 2; }
        } else if (cmd == "vpl") {
            if (a == "-m" || a == "--max-depth") max_depth = val();
            else if (a == "-r" || a == "--rr-depth") rr_depth = val();
            else if (a == "-b" || a == "--clamping") (void)val();           // clamping_factor: never read by the reference
            else if (a == "--nb-vpl") nb_vpl = val();
            else if (a == "-l" || a == "--option-lt") option_lt = val();
            else if (a == "-v" || a == "--option-vpl") option_vpl = val();
            else if (a == "--light-streams") light_streams = val();
            else if (a == "-n") { std::fprintf(stderr, "vpl: -n is ambiguous in the reference (min_depth and nb_vpl share it); use --nb-vpl N\n"); return 2; }
            else { std::fprintf(stderr, "unknown vpl option %s\n", a.c_str()); return 2; }
        } else if (cmd == "vol-primitivies") {
            if (a == "-m" || a == "--max-depth") max_depth = val();
            else if (a == "-n" || a == "--min-depth") (void)val();          // `_min_depth` (cli.rs:697): never read
            else if (a == "-r" || a == "--rr-depth") rr_depth = val();
            else if (a == "--nb-primitive") nb_primitive = val();
            else if (a == "-p" || a == "--primitives") primitives = val();
            else if (a == "--radius") radius = val();
            else if (a == "--light-streams") light_streams = val();
            else if (a == "--tree-build") tree_build = val();
            else { std::fprintf(stderr, "unknown vol-primitivies option %s\n", a.c_str()); return 2; }
        } else if (cmd == "photon-beams" || cmd == "photon-planes" || cmd == "virtual-ray-lights") {
            if (a == "-m" || a == "--max-depth") max_depth = val();
            else if (a == "-n" || a == "--min-depth") (void)val();          // `_min_depth` (cli.rs:697): never read
            else if (a == "-r" || a == "--rr-depth") rr_depth = val();
            else if (a == "--nb-primitive") nb_primitive = val();
            else if (a == "--radius") radius = val();
            else if (a == "--light-streams") light_streams = val();
            else { std::fprintf(stderr, "unknown %s option %s\n", cmd.c_str(), a.c_str()); return 2; }
        } else if (cmd == "plane-single") {
            if (a == "-n" || a == "--nb-primitive") plane_nb = val();
            else if (a == "-s" || a == "--strategy") plane_strategy = val();
            else if (a == "--uncorrelated") plane_uncorrelated = true;
            else { std::fprintf(stderr, "unknown plane-single option %s\n", a.c_str()); return 2; }
        } else if (cmd == "point-normal-mis") {
            if (a == "-s" || a == "--strategy") pn_strategy = val();
            else if (a == "-z" || a == "--disable-aa") pn_disable_aa = true;
            else if (a == "-x" || a == "--use-mis") { if (pn_unbuilt.empty()) pn_unbuilt = a; }
            else if (a == "-k" || a == "--splitting" || a == "-w" || a == "--warps" || a == "--warps-strategy") { (void)val(); if (pn_unbuilt.empty()) pn_unbuilt = a; }
            else { std::fprintf(stderr, "unknown point-normal-mis option %s\n", a.c_str()); return 2; }
        } else if (cmd == "point-normal") {
            if (a == "-s" || a == "--strategy") pn_strategy = val();
            else if (a == "-z" || a == "--disable-aa") pn_disable_aa = true;
            else if (a == "-x" || a == "--use-mis") { if (pn_unbuilt.empty()) pn_unbuilt = a; }
            else if (a == "-k" || a == "--splitting" || a == "-w" || a == "--warps" || a == "--warps-strategy") { (void)val(); if (pn_unbuilt.empty()) pn_unbuilt = a; }
            else { std::fprintf(stderr, "unknown point-normal option %s\n", a.c_str()); return 2; }
        } else if (cmd == "light-tracing") {
            if (a == "-m" || a == "--max-depth") max_depth = val();
            else if (a == "-n" || a == "--min-depth") min_depth = val();
            else if (a == "-r" || a == "--rr-depth") rr_depth = val();
            else if (a == "-s" || a == "--strategy") strategy = val();
            else { std::fprintf(stderr, "unknown light-tracing option %s\n", a.c_str()); return 2; }
        } else {
            if (a == "-m" || a == "--max-depth") max_depth = val();
            else if (a == "-n" || a == "--min-depth") min_depth = val();
            else if (a == "-r" || a == "--rr-depth") rr_depth = val();
            else if (a == "-x" || a == "--single-scattering") single_scattering = true;
            else if (a == "-s" || a == "--strategy") strategy = val();
            else { std::fprintf(stderr, "unknown path option %s\n", a.c_str()); return 2; }
        }
    }
    if (scene_path.empty() || output.empty() || !have_cmd) {
        std::fprintf(stderr, "usage: rustlight-amd <scene.pbrt|scene.xml> -n SPP -o out.pfm [-r independent[:SEED]|stratified[:SEED]] [-m s[:a[:g]]] path [-m max] [-n min] [-r rr] [-x] [-s all|bsdf|emitter]\n");
        return 2;
    }
    // A light-pass command runs on the independent sampler, one kind of streams (`streams`: per-sample for light-tracing, reference order for the gathers), exact
    // numerics and one device, and all but light-tracing (`one_pass`) in one pass: what it cannot do is refused here, before a device is opened
    auto refused = [&](const char* name, rl_stream_mode streams, bool one_pass) -> bool {
        const char* why = nullptr;
        if (rng == "stratified" || rng.rfind("stratified:", 0) == 0) why = "-r stratified is not supported (independent[:SEED] only)";
        else if (mode_given && mode != streams) why = streams == RL_STREAM_PER_SAMPLE ? "--stream-mode reference is not supported (light paths use per-sample streams)" : "--stream-mode per-sample is not supported (the gather uses reference-order streams)";
        else if (numerics == RL_NUMERICS_FAST) why = "--numerics fast is not supported";
        else if (gpus > 1) why = "--gpus > 1 is not supported";
        else if (one_pass && (!average.empty() || !equal_time.empty())) why = "-a / -e are not supported";
        else if (one_pass && frames_in_flight > 1) why = "--frames-in-flight is not supported";
        if (why) std::fprintf(stderr, "%s: %s\n", name, why);
        return why != nullptr;
    };
    IntegratorLightTracing light;
    if (cmd == "light-tracing") {
        if (refused("light-tracing", RL_STREAM_PER_SAMPLE, false)) return 2;
        if (strategy == "all") light.strategy = RL_LIGHT_ALL;
        else if (strategy == "surface") light.strategy = RL_LIGHT_SURFACE;
        else if (strategy == "volume") light.strategy = RL_LIGHT_VOLUME;
        else { std::fprintf(stderr, "invalid light-tracing strategy: %s (all, surface or volume)\n", strategy.c_str()); return 2; }
        light.max_depth = match_infinity(max_depth);
        light.min_depth = match_infinity(min_depth);
        light.rr_depth = match_infinity(rr_depth);
        light.device = device;
        light.options = options;
    }
    // vpl, vol-primitivies, photon-beams, photon-planes, virtual-ray-lights: how the light paths draw (the gather stays in reference order either way)
    LightStreams light_streams_mode = LightStreams::Reference;
    if (cmd == "vpl" || cmd == "vol-primitivies" || cmd == "photon-beams" || cmd == "photon-planes" || cmd == "virtual-ray-lights") {
        if (light_streams == "per-path") light_streams_mode = LightStreams::PerPath;
        else if (light_streams != "reference") { std::fprintf(stderr, "invalid --light-streams: %s (reference or per-path)\n", light_streams.c_str()); return 2; }
    }
    IntegratorVPL vpl;
    if (cmd == "vpl") {
        auto option = [](const std::string& v, rl_vpl_option* out) {
            if (v == "all") *out = RL_VPL_ALL; else if (v == "surface") *out = RL_VPL_SURFACE; else if (v == "volume") *out = RL_VPL_VOLUME; else return false;
            return true;
        };
        if (refused("vpl", RL_STREAM_REFERENCE_ORDER, true)) return 2;
        if (!option(option_lt, &vpl.option_lt)) { std::fprintf(stderr, "invalid vpl -l option: %s (all, surface or volume)\n", option_lt.c_str()); return 2; }
        if (!option(option_vpl, &vpl.option_vpl)) { std::fprintf(stderr, "invalid vpl -v option: %s (all, surface or volume)\n", option_vpl.c_str()); return 2; }
        if (!parse_count("--nb-vpl", nb_vpl, &vpl.nb_vpl)) return 2;
        vpl.max_depth = match_infinity(max_depth);
        vpl.rr_depth = match_infinity(rr_depth);
        vpl.light_streams = light_streams_mode;
        vpl.device = device;
        vpl.options = options;
    }
    // vol-primitivies: the primitives that are not built are refused here
    auto parse_radius = [&](float* out) -> bool {
        char* end = nullptr;
        *out = std::strtof(radius.c_str(), &end);
        if (radius.empty() || *end != '\0' || !(*out > 0.0f) || *out > 3.0e38f) { std::fprintf(stderr, "invalid --radius: %s (a finite number > 0)\n", radius.c_str()); return false; }
        return true;
    };
    IntegratorVolPrimitives volp;
    if (cmd == "vol-primitivies") {
        if (primitives == "beam" || primitives == "plane" || primitives == "vrl") { std::fprintf(stderr, "vol-primitivies: -p %s is not built (bre only)\n", primitives.c_str()); return 2; }
        if (primitives != "bre") { std::fprintf(stderr, "%s is not a correct primitive (bre, beam, plane, vrl)\n", primitives.c_str()); return 2; }
        if (refused("vol-primitivies", RL_STREAM_REFERENCE_ORDER, true)) return 2;
        if (!parse_count("--nb-primitive", nb_primitive, &volp.nb_primitive)) return 2;
        if (!parse_radius(&volp.radius)) return 2;
        volp.max_depth = match_infinity(max_depth);
        volp.rr_depth = match_infinity(rr_depth);
        volp.light_streams = light_streams_mode;
        if (tree_build == "device") volp.tree_build = TreeBuild::Device;
        else if (tree_build != "host") { std::fprintf(stderr, "invalid --tree-build: %s (host or device)\n", tree_build.c_str()); return 2; }
        volp.device = device;
        volp.options = options;
    }
    // photon-beams, virtual-ray-lights, photon-planes: the limits of vol-primitivies, and the medium the reference panics without; photon-planes also has the
    // depth below which no plane exists (min_max_depth)
    auto fill_beam_pass = [&](const char* name, auto& it, uint32_t min_max_depth) -> bool {
        if (refused(name, RL_STREAM_REFERENCE_ORDER, true)) return false;
        if (!parse_count("--nb-primitive", nb_primitive, &it.nb_primitive)) return false;
        if (it.nb_primitive > (uint32_t)RL_BEAM_MAX) { std::fprintf(stderr, "invalid --nb-primitive: %s (1 .. %d)\n", nb_primitive.c_str(), (int)RL_BEAM_MAX); return false; }
        if (!parse_radius(&it.radius)) return false;
        const Medium m = parse_medium(medium);
        if (m.sigma_a + m.sigma_s == 0.0f) { std::fprintf(stderr, "%s: the integrator needs a medium (add -m SIGMA_S[:SIGMA_A[:G]])\n", name); return false; }
        it.max_depth = match_infinity(max_depth);
        if (it.max_depth.has_value() && *it.max_depth < min_max_depth) {
            std::fprintf(stderr, "%s: -m %s is too small (no light path holds a plane below a max depth of %u)\n", name, max_depth.c_str(), min_max_depth);
            return false;
        }
        it.rr_depth = match_infinity(rr_depth);
        it.light_streams = light_streams_mode;
        it.device = device;
        it.options = options;
        return true;
    };
    IntegratorPhotonBeams pbeams;
    if (cmd == "photon-beams" && !fill_beam_pass("photon-beams", pbeams, 0u)) return 2;
    IntegratorVirtualRayLights vrls;
    if (cmd == "virtual-ray-lights" && !fill_beam_pass("virtual-ray-lights", vrls, 0u)) return 2;
    IntegratorPhotonPlanes pplanes;
    if (cmd == "photon-planes" && !fill_beam_pass("photon-planes", pplanes, 4u)) return 2;
    // plane-single needs the medium
    IntegratorSinglePlane plane;
    if (cmd == "plane-single") {
        static const char* const names[] = {"uv", "vt", "ut", "average", "discrete_mis", "ualpha", "cmis"};      // rl_plane_strategy, by value
        int which = -1;
        for (int k = 0; k < 7; k++) if (plane_strategy == names[k]) which = k;
        if (which < 0) { std::fprintf(stderr, "%s is not a correct strategy choice (uv, ut, vt, average, discrete_mis, valpha, cmis)\n", plane_strategy.c_str()); return 2; }
        plane.strategy = (rl_plane_strategy)which;
        if (refused("plane-single", RL_STREAM_REFERENCE_ORDER, true)) return 2;
        if (!parse_count("--nb-primitive", plane_nb, &plane.nb_primitive)) return 2;
        // "Volume integrator need a volume (add -m )": the medium string as the scene setup below parses it
        const Medium m = parse_medium(medium);
        if (m.sigma_a + m.sigma_s == 0.0f) { std::fprintf(stderr, "plane-single: the integrator needs a medium (add -m SIGMA_S[:SIGMA_A[:G]])\n"); return 2; }
        plane.device = device;
        plane.options = options;
    }
    // point-normal: the seven plain strategies on either kind of streams; everything else of the reference's subcommand is refused by name.
    // point-normal-mis: the same names and refusals, the MIS estimator of the name's distance family
    IntegratorPointNormal pn;
    IntegratorPointNormalMis pnmis;
    if (cmd == "point-normal" || cmd == "point-normal-mis") {
        const char* const word = cmd.c_str();
        static const char* const names[] = {"tr_ex", "tr_phase", "eq_ex", "eq_phase", "eq_clamped_ex", "eq_clamped_phase", "pn_ex"};      // rl_pn_strategy, by value
        static const char* const flavoured[] = {"eq_best_ex", "eq_warp_ex", "eq_phase_taylor_ex", "eq_tr_taylor_ex", "eq_clamped_best_ex", "eq_clamped_warp_ex",
                                                "eq_clamped_phase_taylor_ex", "eq_clamped_tr_taylor_ex", "pn_tr_taylor_ex", "pn_phase_taylor_ex", "pn_warp_ex", "pn_best_ex"};
        const char* list = "tr_ex, tr_phase, eq_ex, eq_phase, eq_clamped_ex, eq_clamped_phase, pn_ex";
        for (const char* f : flavoured)
            if (pn_strategy == f) { std::fprintf(stderr, "%s: -s %s is not built (%s)\n", word, f, list); return 2; }
        int which = -1;
        for (int k = 0; k < 7; k++) if (pn_strategy == names[k]) which = k;
        if (which < 0) { std::fprintf(stderr, "invalid strategy: %s (%s)\n", pn_strategy.c_str(), list); return 2; }
        if (!pn_unbuilt.empty() && cmd == "point-normal") { std::fprintf(stderr, "point-normal: %s is not built (MIS, splitting and the warps are left out)\n", pn_unbuilt.c_str()); return 2; }
        if (!pn_unbuilt.empty()) { std::fprintf(stderr, "point-normal-mis: %s is not built (the subcommand is `point-normal -x` itself; splitting and the warps are left out)\n", pn_unbuilt.c_str()); return 2; }
        if (use_ats) { std::fprintf(stderr, "%s: -x ats is not built (the light tree's emitter sampling is left out)\n", word); return 2; }
        if (refused(word, mode, true)) return 2;
        const Medium m = parse_medium(medium);
        if (m.sigma_a + m.sigma_s == 0.0f) { std::fprintf(stderr, "%s: the integrator needs a medium (add -m SIGMA_S[:SIGMA_A[:G]])\n", word); return 2; }
        pn.strategy = (rl_pn_strategy)which;
        pn.use_aa = !pn_disable_aa;
        pn.stream_mode = mode;
        pn.device = device;
        pn.options = options;
        pnmis.strategy = pn.strategy; pnmis.use_aa = pn.use_aa; pnmis.stream_mode = mode; pnmis.device = device; pnmis.options = options;
    }
    IntegratorSinglePlaneUncorrelated uplane;
    uplane.nb_primitive = plane.nb_primitive; uplane.strategy = plane.strategy; uplane.device = device; uplane.options = options;
    // the sampler (cli.rs:876-896): the master sampler that draws the block seeds is IndependentSampler(SEED) for both kinds — OS entropy without a seed, as
    // IndependentSampler::default() / StratifiedSampler's random() are; `stratified:SEED` is this drop-in's reproducible form.  stratified =
    // RL_STREAM_STRATIFIED: StratifiedSampler::create(spp, 4) on every pixel (include/rustlight_amd.h)
    uint64_t seed = 0;
    {
        auto parse_seed = [&](const char* t) -> bool {
            if (!*t || *t == '-' || *t == '+' || *t == ' ') return false;
            char* e = nullptr;
            errno = 0;
            const unsigned long long v = std::strtoull(t, &e, 10);
            if (errno == ERANGE || !e || *e) return false;
            seed = v;
            return true;
        };
        if (rng == "independent") seed = std::random_device{}();   // IndependentSampler::default(): OS entropy
        else if (rng.rfind("independent:", 0) == 0) seed = std::strtoull(rng.c_str() + 12, nullptr, 10);
        else if (rng == "stratified" || rng.rfind("stratified:", 0) == 0) {
            if (rng == "stratified") seed = std::random_device{}();
            else if (!parse_seed(rng.c_str() + 11)) { std::fprintf(stderr, "stratified sampler: the seed must be an unsigned 64-bit integer (got %s)\n", rng.c_str() + 11); return 2; }
            if (mode_given) { std::fprintf(stderr, "-r stratified sets the stream mode itself: it cannot be combined with --stream-mode\n"); return 2; }
            if (numerics == RL_NUMERICS_FAST) { std::fprintf(stderr, "-r stratified is not built with --numerics fast\n"); return 2; }
            mode = RL_STREAM_STRATIFIED;
            size_t power_of4 = 1;
            while (power_of4 < nbsamples) power_of4 *= 4;
            if (power_of4 != nbsamples) std::fprintf(stderr, "WARN %zu is not 4 multiple (increase count to %zu), the stratified sampler will be less efficient!\n", nbsamples, power_of4);
        }
        else { std::fprintf(stderr, "Wrong sampler type provided %s (independent[:seed] or stratified[:seed])\n", rng.c_str()); return 2; }
    }
    try {
        std::unique_ptr<Scene> scene(Scene::load(scene_path, shading_normals));
        scene->nb_samples = nbsamples;
        scene->output_img_path = output;
        const Medium m = parse_medium(medium);
        if (m.n_parts > 3) { std::fprintf(stderr, "invalid medium_density\n"); return 2; }
        if (m.sigma_a + m.sigma_s != 0.0f) {
            float sa[3] = {m.sigma_a, m.sigma_a, m.sigma_a}, s3[3] = {m.sigma_s, m.sigma_s, m.sigma_s};
            if (rl_scene_set_medium(scene->handle, sa, s3, m.n_parts > 2 ? RL_PHASE_HG : RL_PHASE_ISOTROPIC, m.g) != RL_OK) { std::fprintf(stderr, "invalid medium_density\n"); return 2; }
        }
        if (scale_image != 1.0f && rl_scene_scale_image(scene->handle, scale_image) != RL_OK) { std::fprintf(stderr, "invalid image scale: %s\n", rl_last_error()); return 2; }
        if (light_override != RL_EMISSION_COLOR) {   // "Overide light is needed" (cli.rs:410-429): every light mesh becomes HSV { scale } / Texture { scale, butterfly.jpg }
            int bitmap = -1;
            if (light_override == RL_EMISSION_TEXTURE) {
                uint32_t bw = 0, bh = 0;
                if (rl_load_image("butterfly.jpg", &bw, &bh, nullptr, 0) != RL_OK) { std::fprintf(stderr, "texture-light: cannot read butterfly.jpg from the working directory (Bitmap::read(\"butterfly.jpg\"), cli.rs:423): %s\n", rl_last_error()); return 1; }
                std::vector<float> px((size_t)3 * bw * bh);
                if (rl_load_image("butterfly.jpg", &bw, &bh, px.data(), px.size()) != RL_OK) { std::fprintf(stderr, "texture-light: %s\n", rl_last_error()); return 1; }
                bitmap = rl_scene_add_bitmap(scene->handle, bw, bh, px.data());
                if (bitmap < 0) { std::fprintf(stderr, "texture-light: %s\n", rl_last_error()); return 1; }      // (a negative return is an error code, not a bitmap id)
            }
            if (rl_scene_override_light_emission(scene->handle, light_override, bitmap) != RL_OK) { std::fprintf(stderr, "-x %s: %s\n", light_override == RL_EMISSION_HSV ? "hvs-light" : "texture-light", rl_last_error()); return 1; }
        }
        scene->build_emitters(use_ats);      // scene.build_emitters(use_ats) (cli.rs:432)
        IntegratorPathTracing integrator;
        if (cmd == "light-tracing" || cmd == "vpl" || cmd == "vol-primitivies" || cmd == "photon-beams" || cmd == "photon-planes" || cmd == "virtual-ray-lights" || cmd == "plane-single" || cmd == "point-normal" || cmd == "point-normal-mis") strategy = "all";       // (the path integrator below is not used)
        integrator.min_depth = match_infinity(min_depth);
        integrator.max_depth = match_infinity(max_depth);
        integrator.rr_depth = match_infinity(rr_depth);
        if (strategy == "all") integrator.strategy = IntegratorPathTracingStrategies::All;
        else if (strategy == "bsdf") integrator.strategy = IntegratorPathTracingStrategies::BSDF;
        else if (strategy == "emitter") integrator.strategy = IntegratorPathTracingStrategies::Emitter;
        else { std::fprintf(stderr, "invalid strategy: %s\n", strategy.c_str()); return 2; }
        integrator.single_scattering = single_scattering;
        integrator.device = device;
        integrator.n_gpus = gpus;      // --gpus N: blocks dealt round-robin over N devices, one RCCL reduce of the framebuffers over xGMI
        integrator.stream_mode = mode;
        integrator.numerics = numerics;
        integrator.frames_in_flight = frames_in_flight;
        integrator.options = options;
        IndependentSampler sampler(seed);
        BufferCollection img;
        double elapsed_ms = 0.0;
        if (cmd == "ao") {
            IntegratorAO ao;
            ao.device = device; ao.stream_mode = mode; ao.normal_correction = ao_normal_correction;
            if (ao_distance == "inf") ao.max_distance = std::nullopt; else ao.max_distance = std::strtof(ao_distance.c_str(), nullptr);
            img = ao.compute(sampler, *scene); elapsed_ms = ao.last_stats.render_ms;
        } else if (cmd == "direct") {
            IntegratorDirect di;
            di.device = device; di.stream_mode = mode; di.nb_bsdf_samples = nb_bsdf; di.nb_light_samples = nb_light;
            img = di.compute(sampler, *scene); elapsed_ms = di.last_stats.render_ms;
        } else if (cmd == "vpl") {
            img = vpl.compute(sampler, *scene); elapsed_ms = vpl.last_stats.render_ms;
        } else if (cmd == "vol-primitivies") {
            img = volp.compute(sampler, *scene); elapsed_ms = volp.last_stats.render_ms;
        } else if (cmd == "photon-beams") {
            img = pbeams.compute(sampler, *scene); elapsed_ms = pbeams.last_stats.render_ms;
        } else if (cmd == "photon-planes") {
            img = pplanes.compute(sampler, *scene); elapsed_ms = pplanes.last_stats.render_ms;
        } else if (cmd == "virtual-ray-lights") {
            img = vrls.compute(sampler, *scene); elapsed_ms = vrls.last_stats.render_ms;
        } else if (cmd == "plane-single") {
            if (plane_uncorrelated) { img = uplane.compute(sampler, *scene); elapsed_ms = uplane.last_stats.render_ms; }
            else { img = plane.compute(sampler, *scene); elapsed_ms = plane.last_stats.render_ms; }
        } else if (cmd == "point-normal") {
            img = pn.compute(sampler, *scene); elapsed_ms = pn.last_stats.render_ms;
        } else if (cmd == "point-normal-mis") {
            img = pnmis.compute(sampler, *scene); elapsed_ms = pnmis.last_stats.render_ms;
        } else if (cmd == "light-tracing") {
            if (!equal_time.empty()) {
                IntegratorEqualTime<IntegratorLightTracing> eq{light, std::strtod(equal_time.c_str(), nullptr) * 1000.0};
                img = eq.compute(sampler, *scene);
                std::fprintf(stderr, "INFO Number iter: %zu\nINFO Number spp: %zu\n", eq.iterations, eq.iterations * scene->nb_samples);
            } else if (!average.empty()) {
                IntegratorAverage<IntegratorLightTracing> av{light, std::nullopt, true};
                if (average != "inf") av.time_out = (size_t)std::strtoull(average.c_str(), nullptr, 10);
                img = av.compute(sampler, *scene);
            } else img = light.compute(sampler, *scene);
            elapsed_ms = light.last_stats.render_ms;
        } else if (!equal_time.empty()) {        // cli.rs:898-907
            IntegratorEqualTime<IntegratorPathTracing> eq{integrator, std::strtod(equal_time.c_str(), nullptr) * 1000.0};
            img = eq.compute(sampler, *scene); elapsed_ms = integrator.last_stats.render_ms;
            std::fprintf(stderr, "INFO Number iter: %zu\nINFO Number spp: %zu\n", eq.iterations, eq.iterations * scene->nb_samples);
        } else if (!average.empty()) {           // cli.rs:908-917
            IntegratorAverage<IntegratorPathTracing> av{integrator, std::nullopt, true};
            if (average != "inf") av.time_out = (size_t)std::strtoull(average.c_str(), nullptr, 10);
            img = av.compute(sampler, *scene); elapsed_ms = integrator.last_stats.render_ms;
        } else { img = integrator.compute(sampler, *scene); elapsed_ms = integrator.last_stats.render_ms; }
        std::fprintf(stderr, "INFO Elapsed Integrator: %.0f ms\n", elapsed_ms);
        if (integrator.multi) {     // --gpus N: where the shards ran, how the framebuffers were merged, kernel ms per device
            std::vector<char> buf(1 << 16);
            if (rl_multi_describe(integrator.multi, buf.data(), buf.size()) == RL_OK) std::fprintf(stderr, "INFO Multi-GPU: %s\n", buf.data());
            for (int g = 0; g < gpus; g++) {
                int dev = -1; rl_render_stats st{};
                if (rl_multi_shard_stats(integrator.multi, g, &dev, &st) == RL_OK)
                    std::fprintf(stderr, "INFO shard %d on device %d: kernel %.2f ms (chain pass %.2f ms), %llu camera samples\n", g, dev, st.ms_other + st.ms_prepass, st.ms_prepass, (unsigned long long)st.camera_samples);
            }
        }
        std::fprintf(stderr, "INFO Save final image: %s\n", output.c_str());
        img.save("primal", output);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "ERROR %s\n", e.what());
        return 1;
    }
    return 0;
}
