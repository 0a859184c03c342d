"""Writes tests/golden/cli_refusals.json: a corpus of `rustlight-amd` command lines that the CLI refuses before it opens a device, each with its exit code and
its exact stderr, recorded from the built CLI.  tests/test_cli_refusals.py holds the CLI to it byte for byte, so a change of cli.cpp's control flow cannot move
a message, an exit code or the order in which two faults of one line are reported.  The corpus: every refused line of the tests/test_*_args.py files and of
test_abi.py's CLI block, the usage line, the missing values, the subcommands without an args file (path, ao, direct), what the scene setup refuses, the two
exit-1 lines that need no device, and the two-fault lines that pin the order of the refusals.  No line reaches the device or the entropy of a seedless sampler:
the file is the same on a machine with a GPU and on one without.  In the file {SCENE} stands for data/cbox.pbrt and {TMP} for the directory the line ran in.
usage: python tests/golden/make_cli_refusals.py      (a few seconds, no GPU; record it before cli.cpp changes, not after)"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cli_refusals.json")
SCENE, TMP = "{SCENE}", "{TMP}"
OUTPUT = ("-o", TMP + "/out.pfm")
BEAM_MAX = 1 << 17
FLAVOURED = ("eq_best_ex", "eq_warp_ex", "eq_phase_taylor_ex", "eq_tr_taylor_ex", "eq_clamped_best_ex", "eq_clamped_warp_ex", "eq_clamped_phase_taylor_ex",
             "eq_clamped_tr_taylor_ex", "pn_tr_taylor_ex", "pn_phase_taylor_ex", "pn_warp_ex", "pn_best_ex")
# what every light-pass subcommand refuses among the global options (point-normal takes both stream modes, light-tracing more than one pass)
LIMITS = (("-r", "stratified:3"), ("--stream-mode", "per-sample"), ("--numerics", "fast"), ("--gpus", "2"), ("-a", "3"), ("-e", "3"), ("--frames-in-flight", "2"))
RADII = ("0", "-0.1", "nan", "inf", "0.1x")
NO_MEDIUM = ((), ("-m", "0.0"), ("-m", "0:0"))


def line(*args, spp="2", medium=("-m", "1.0")):
    """The command line of the args files' helpers: the scene, -n, the medium, -o, then `args`."""
    return [SCENE, "-n", spp, *medium, *OUTPUT, *args]


def plain(*args):
    """... of the helpers without a medium (light-tracing, vpl, the stratified sampler)."""
    return line(*args, spp="4", medium=())


def corpus():
    c = []
    # the usage line, a second positional word, missing values
    c += [[*OUTPUT, "path"], [SCENE, "path"], [SCENE, *OUTPUT], [], line("also.pbrt", "path"), line("photon-beam"), line("uncorrelated-plane-single")]
    c += [line("photon-plane"), line("virtual-ray-light"), line("point_normal"), line("point_normal_mis")]
    c += [[SCENE, "-n"], [SCENE, *OUTPUT, "-t"], [SCENE, *OUTPUT, "-l"], [SCENE, *OUTPUT, "--option"], line("path", "-m"), line("ao", "-d"), line("direct", "-b")]
    c += [line("vpl", "--nb-vpl"), line("vol-primitivies", "--tree-build"), line("photon-planes", "--radius"), line("plane-single", "-s"), line("point-normal", "-k")]
    c += [line("point-normal-mis", "--strategy"), line("light-tracing", "-r"), line("virtual-ray-lights", "-n")]
    # path, ao, direct and the options before the subcommand
    c += [line("path", "--bogus"), line("ao", "-m", "3"), line("direct", "-n"), line("path", "ao"), line("path", "-m", "12x"), line("path", "-n", "x"), line("path", "-r", "-"),
          line("path", "-s", "nope"), line("path", "-s", "surface"), line("path", "-m", "12x", "-s", "nope"), line("path", medium=("-m", "1:2:3:4")), line("-s", "0", "path"),
          line("-s", "-1", "path"), line("-s", "nan", "path"), line("--bogus", "path"), line("-x", "no-such-option", "path"), line("-z", "path"),
          [SCENE, "-x", "no-such-option", "-n", "1", *OUTPUT, "path"], [SCENE, "path", "--bogus"], line("path", medium=("-m", "1:2:3:4"), spp="0")]
    c += [line("-r", "bogus", "path", "-m", "12x"), line("path", "-m", "12x", medium=("-m", "1:2:3:4")), line("-r", "bogus", "path", medium=("-m", "1:2:3:4"))]
    c += [[TMP + "/missing.pbrt", "-n", "2", *OUTPUT, "path"], [TMP + "/missing.pbrt", "-n", "2", "-r", "bogus", *OUTPUT, "path"], line("-x", "texture-light", "path")]
    # the stratified sampler
    c += [plain("-r", "stratified:abc", "path"), plain("-r", "stratified:-1", "ao"), plain("-r", "stratified:", "ao"), plain("-r", "stratified:18446744073709551616", "ao"),
          plain("-r", "stratified", "--stream-mode", "per-sample", "path"), plain("--stream-mode", "reference", "-r", "stratified:3", "direct"),
          plain("-r", "stratified:7", "--numerics", "fast", "path"), plain("-r", "bogus", "path"), plain("-r", "stratified:3", "--numerics", "fast", "--stream-mode", "reference", "path"),
          plain("-r", "stratified:+1", "direct"), plain("-r", "stratified: 1", "path"), plain("-r", "independent:", "--stream-mode", "reference", "-r", "stratified:x", "ao")]
    # --light-streams and --tree-build: before the subcommand, under one that lacks it, with a value that is none
    for flag, value in (("--light-streams", "per-path"), ("--tree-build", "device")):
        c += [line(flag, value, cmd) for cmd in ("vpl", "vol-primitivies", "photon-beams", "photon-planes", "virtual-ray-lights", "path")]
        c += [line(cmd, flag, value) for cmd in ("path", "ao", "direct", "light-tracing", "plane-single", "point-normal", "point-normal-mis")]
        c += [line(cmd, flag) for cmd in ("path", "vpl", "vol-primitivies", "photon-beams")]
    c += [line(cmd, "--tree-build", "device") for cmd in ("vpl", "photon-beams", "photon-planes", "virtual-ray-lights")] + [line("ao", "--tree-build", "host")]
    c += [line("direct", "--light-streams", "reference"), line("plane-single", "--uncorrelated", "--light-streams", "per-path"), line("plane-single", "--uncorrelated", "--tree-build", "device")]
    c += [line(cmd, "--light-streams", v) for cmd in ("vpl", "vol-primitivies", "vol-primitives", "photon-beams", "photon-planes", "virtual-ray-lights")
          for v in ("per-sample", "per_path", "parallel", "other", "")]
    c += [line(cmd, "--tree-build", v) for cmd in ("vol-primitivies", "vol-primitives") for v in ("bogus", "", "gpu")]
    c += [line("--stream-mode", "per-sample", cmd, "--light-streams", "per-path") for cmd in ("vpl", "vol-primitivies")]
    # light-tracing
    c += [plain(*g, "light-tracing") for g in (("-r", "stratified:3"), ("-r", "stratified"), ("--stream-mode", "reference"), ("--numerics", "fast"), ("--gpus", "2"))]
    c += [plain("light-tracing", "-s", "bsdf"), plain("light-tracing", "-s", "emitter"), plain("light-tracing", "-x"), plain("light-tracing", "-m", "12x"),
          plain("light-tracing", "-n", "x"), plain("light-tracing", "-r", "1.5"), plain("light-tracing", "-s", "bsdf", "-m", "12x"), plain("--gpus", "2", "light-tracing", "-s", "bsdf"),
          plain("-r", "bogus", "light-tracing", "-m", "12x"), plain("-r", "bogus", "light-tracing")]
    # vpl
    c += [plain(*g, "vpl") for g in LIMITS]
    c += [plain("vpl", "-n", "16"), plain("vpl", "-l", "bsdf"), plain("vpl", "-v", "emitter"), plain("vpl", "--nb-vpl", "0"), plain("vpl", "--nb-vpl", "12x"),
          plain("vpl", "--nb-vpl", str(1 << 21)), plain("vpl", "--nb-vpl", ""), plain("vpl", "-s", "all"), plain("vpl", "-b", "0.5", "-s", "all"), plain("vpl", "-b"),
          plain("--gpus", "2", "vpl", "--light-streams", "other"), plain("--gpus", "2", "vpl", "-l", "bsdf"), plain("vpl", "-l", "bsdf", "-v", "emitter"),
          plain("vpl", "-v", "emitter", "--nb-vpl", "0"), plain("vpl", "--nb-vpl", "0", "-m", "12x"), plain("vpl", "-m", "12x", "-r", "13x"), plain("vpl", "-r", "13x"),
          plain("-t", "4", "-l", "log.txt", "--gpus", "2", "vpl"), plain("-r", "bogus", "vpl", "--nb-vpl", "0")]
    # vol-primitivies (the beam radiance estimate) and its alias
    c += [line(*g, "vol-primitivies") for g in LIMITS]
    c += [line(cmd, "-p", p) for cmd in ("vol-primitivies", "vol-primitives") for p in ("beam", "plane", "vrl", "BRE", "")]
    c += [line("vol-primitivies", "--nb-primitive", n) for n in ("0", "12x", str(1 << 21), str((1 << 20) + 1), "-1")] + [line("vol-primitivies", "--radius", r) for r in RADII]
    c += [line("vol-primitivies", "-s", "all"), line("vol-primitivies", "-n", "3", "-s", "all"), line("vol-primitives", "-x"), line("--gpus", "2", "vol-primitivies", "-p", "beam"),
          line("vol-primitivies", "-p", "nope", "--light-streams", "other"), line("vol-primitivies", "--nb-primitive", "0", "--radius", "0"),
          line("vol-primitivies", "--tree-build", "bogus", "--radius", "0"), line("vol-primitivies", "--tree-build", "bogus", "-m", "12x"),
          line("vol-primitivies", "--radius", "0", "-m", "12x"), line("--gpus", "2", "vol-primitivies", "--nb-primitive", "0"), line("-r", "bogus", "vol-primitivies", "--tree-build", "x")]
    # the three beam-pass subcommands
    for cmd in ("photon-beams", "photon-planes", "virtual-ray-lights"):
        c += [line(*g, cmd) for g in LIMITS]
        c += [line(cmd, "--nb-primitive", n) for n in ("0", "12x", str(BEAM_MAX + 1), str(1 << 21))] + [line(cmd, "--radius", r) for r in RADII]
        c += [line(cmd, "-p", "beam"), line(cmd, "-p", "plane"), line(cmd, "-p", "vrl"), line(cmd, "-s", "all"), line(cmd, "-n", "3", "-s", "all"), line(cmd, "-m", "12x"), line(cmd, "-r", "12x"),
              line(cmd, "-m", "12x", "-r", "13x"), line(cmd, "--radius", "0", "-m", "3")]
        c += [line(cmd, medium=m) for m in NO_MEDIUM] + [line(cmd, "--radius", "0", medium=()), line(cmd, "-m", "12x", medium=()), line("--gpus", "2", cmd, "--nb-primitive", "0"),
                                                        line("--gpus", "2", cmd, "--light-streams", "other"), line("-r", "bogus", cmd, "--radius", "0"), line("-r", "bogus", cmd, medium=())]
    c += [line("photon-planes", "-m", "3"), line("photon-planes", "-m", "1"), line("photon-planes", "-m", "0"), line("photon-planes", "-m", "3", "-r", "12x"),
          line("photon-planes", "-m", "3", medium=())]
    # plane-single, with and without --uncorrelated
    for cmd in (("plane-single",), ("plane-single", "--uncorrelated")):
        c += [line(*g, *cmd) for g in LIMITS]
        c += [line(*cmd, "-s", "valpha"), line("plane-single", "--strategy", "AVERAGE", *cmd[1:]), line(*cmd, "-s", ""), line(*cmd, "-n", "0"), line("plane-single", "--nb-primitive", "12x", *cmd[1:]),
              line(*cmd, "-n", str((1 << 20) + 1)), line(*cmd, "-m", "3"), line(*cmd, "-p", "plane"), line(*cmd, "--uncorrelated=1"), line("--gpus", "2", *cmd, "-s", "valpha"),
              line("--gpus", "2", *cmd, "-n", "0"), line("-r", "bogus", *cmd, "-n", "0")]
        c += [line(*cmd, medium=m) for m in NO_MEDIUM] + [line(*cmd, "-n", "0", medium=()), line("--gpus", "2", *cmd, medium=()), line("-r", "bogus", *cmd, medium=())]
    c += [line("--uncorrelated", "plane-single"), line("path", "--uncorrelated")]
    # point-normal and point-normal-mis
    for cmd in ("point-normal", "point-normal-mis"):
        c += [line(cmd, "-s", name) for name in FLAVOURED] + [line(cmd, "-s", s) for s in ("tr", "pn_phase", "nope", "")] + [line(cmd, "--strategy", "TR_EX")]
        c += [line(cmd, "-x"), line(cmd, "--use-mis"), line(cmd, "-k", "0.5"), line(cmd, "--splitting", "0.5"), line(cmd, "-w", "PT"), line(cmd, "--warps", "N"),
              line(cmd, "--warps-strategy", "B"), line(cmd, "-s", "pn_ex", "-x"), line(cmd, "-s", "pn_ex", "-k", "2"), line(cmd, "-k", "2", "-x"), line(cmd, "-x", "-w", "PT"),
              line("-x", "ats", cmd), line(cmd, "-n", "3"), line(cmd, "-m", "3"), line("-z", cmd)]
        c += [line(*g, cmd) for g in LIMITS if g[0] != "--stream-mode"] + [line("--stream-mode", s, "--gpus", "2", cmd) for s in ("reference", "per-sample")]
        c += [line(cmd, medium=m) for m in NO_MEDIUM]
        # the order: flavoured strategy, invalid strategy, unbuilt option, -x ats, the limits, the medium
        c += [line("-x", "ats", "--gpus", "2", cmd, "-s", "eq_best_ex", "-x", medium=()), line("-x", "ats", "--gpus", "2", cmd, "-s", "nope", "-x", medium=()),
              line("-x", "ats", "--gpus", "2", cmd, "-x", medium=()), line("-x", "ats", "--gpus", "2", cmd, medium=()), line("--gpus", "2", cmd, medium=()), line("-r", "bogus", cmd, medium=())]
    c += [line("path", "-z")]
    return c


def run(exe, args, tmp):
    """One line of the corpus in the directory `tmp`: (exit code, stderr with the two paths written back as their placeholders)."""
    scene = os.path.join(ROOT, "data", "cbox.pbrt")
    argv = [a.replace(SCENE, scene).replace(TMP, tmp) for a in args]
    r = subprocess.run([exe, *argv], capture_output=True, cwd=tmp, timeout=60)
    assert os.listdir(tmp) == [], (args, os.listdir(tmp))
    return r.returncode, r.stderr.decode().replace(scene, SCENE).replace(tmp, TMP)


if __name__ == "__main__":
    from rustlight_amd import api

    exe = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(api.LIB_PATH), "rustlight-amd")
    entries, seen = [], set()
    with tempfile.TemporaryDirectory() as tmp:
        for args in corpus():
            if tuple(args) in seen:
                continue
            seen.add(tuple(args))
            code, err = run(exe, args, tmp)
            assert code in (1, 2) and "no CPU fallback" not in err and "INFO" not in err, (args, code, err)      # a line that got further is no refusal
            entries.append({"args": args, "exit": code, "stderr": err})
    with open(OUT, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e) for e in entries) + "\n]\n")      # one line of the corpus per line of the file
    print(len(entries), "lines;", sum(e["exit"] == 1 for e in entries), "exit 1")
