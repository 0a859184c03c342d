"""`rustlight-amd ... plane-single --uncorrelated`: the argument errors the CLI reports before it opens a device (no GPU needed) and the lines that parse."""
import os
import subprocess

from rustlight_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, "data", "cbox.pbrt")
CMD = ("plane-single", "--uncorrelated")


def _cli(tmp_path, *args, medium=("-m", "1.0")):
    exe = os.path.join(os.path.dirname(api.LIB_PATH), "rustlight-amd")
    return subprocess.run([exe, SCENE, "-n", "2", *medium, "-o", str(tmp_path / "out.pfm"), *args], capture_output=True, text=True, timeout=60)


def test_uncorrelated_argument_errors(built, tmp_path):
    """What plane-single refuses, with its error text, wherever --uncorrelated stands among the subcommand's options."""
    for args, word in (((*CMD, "-s", "valpha"), "valpha is not a correct strategy choice (uv, ut, vt, average, discrete_mis, valpha, cmis)"),
                       (("plane-single", "--strategy", "AVERAGE", "--uncorrelated"), "not a correct strategy choice"),
                       (("-r", "stratified:3", *CMD), "stratified"),
                       (("--stream-mode", "per-sample", *CMD), "per-sample"),
                       (("--numerics", "fast", *CMD), "fast"),
                       (("--gpus", "2", *CMD), "--gpus"),
                       (("-a", "3", *CMD), "-a"),
                       (("-e", "3", *CMD), "-e"),
                       (("--frames-in-flight", "2", *CMD), "--frames-in-flight"),
                       ((*CMD, "-n", "0"), "--nb-primitive"),
                       (("plane-single", "--nb-primitive", "12x", "--uncorrelated"), "--nb-primitive"),
                       ((*CMD, "-n", str((1 << 20) + 1)), "--nb-primitive"),
                       ((*CMD, "--light-streams", "per-path"), "vpl and vol-primitivies only"),
                       ((*CMD, "--tree-build", "device"), "vol-primitivies only"),
                       ((*CMD, "-m", "3"), "plane-single option"),
                       ((*CMD, "--uncorrelated=1"), "plane-single option"),
                       (("--uncorrelated", "plane-single"), "unknown option --uncorrelated"),
                       (("path", "--uncorrelated"), "unknown path option --uncorrelated")):
        r = _cli(tmp_path, *args)
        assert r.returncode == 2 and word in r.stderr and r.stderr.count("\n") == 1, (args, r.stderr)
        assert not os.path.exists(tmp_path / "out.pfm")


def test_uncorrelated_needs_a_medium(built, tmp_path):
    for medium in ((), ("-m", "0.0"), ("-m", "0:0")):
        r = _cli(tmp_path, *CMD, medium=medium)
        assert r.returncode == 2 and "medium" in r.stderr and r.stderr.count("\n") == 1, (medium, r.stderr)
        assert not os.path.exists(tmp_path / "out.pfm")


def test_uncorrelated_options_parse_up_to_the_device(built, tmp_path):
    """Well-formed lines (the defaults, every strategy, both spellings of the options, the flag before and after them) get as far as opening a device: without
    one, the no-fallback refusal."""
    lines = [CMD, (*CMD, "--nb-primitive", "16", "--strategy", "cmis"), ("plane-single", "-n", "4", "--uncorrelated", "-s", "ut")]
    lines += [(*CMD, "-n", "8", "-s", s) for s in api.PLANE_STRATEGIES]
    for args in lines:
        r = _cli(tmp_path, *args)
        if r.returncode == 0:                                  # a machine with a GPU renders it
            assert os.path.exists(tmp_path / "out.pfm")
            os.remove(tmp_path / "out.pfm")
        else:
            assert r.returncode != 2 and "no CPU fallback" in r.stderr, (args, r.stderr)
