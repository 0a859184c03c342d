"""`rustlight-amd ... plane-single`: the argument errors the CLI reports before it opens a device (no GPU needed) and the lines that parse."""
import os
import subprocess

from rustlight_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, "data", "cbox.pbrt")


def _cli(tmp_path, *args, medium=("-m", "1.0")):
    exe = os.path.join(os.path.dirname(api.LIB_PATH), "rustlight-amd")
    return subprocess.run([exe, SCENE, "-n", "2", *medium, "-o", str(tmp_path / "out.pfm"), *args], capture_output=True, text=True, timeout=60)


def test_plane_single_argument_errors(built, tmp_path):
    for args, word in ((("plane-single", "-s", "valpha"), "valpha is not a correct strategy choice (uv, ut, vt, average, discrete_mis, valpha, cmis)"),
                       (("plane-single", "--strategy", "AVERAGE"), "not a correct strategy choice"),
                       (("-r", "stratified:3", "plane-single"), "stratified"),
                       (("--stream-mode", "per-sample", "plane-single"), "per-sample"),
                       (("--numerics", "fast", "plane-single"), "fast"),
                       (("--gpus", "2", "plane-single"), "--gpus"),
                       (("-a", "3", "plane-single"), "-a"),
                       (("-e", "3", "plane-single"), "-e"),
                       (("--frames-in-flight", "2", "plane-single"), "--frames-in-flight"),
                       (("plane-single", "-n", "0"), "--nb-primitive"),
                       (("plane-single", "--nb-primitive", "12x"), "--nb-primitive"),
                       (("plane-single", "-n", str((1 << 20) + 1)), "--nb-primitive"),
                       (("plane-single", "--light-streams", "per-path"), "vpl and vol-primitivies only"),
                       (("plane-single", "--tree-build", "device"), "vol-primitivies only"),
                       (("plane-single", "-m", "3"), "plane-single option"),
                       (("plane-single", "-p", "plane"), "plane-single option")):
        r = _cli(tmp_path, *args)
        assert r.returncode == 2 and word in r.stderr and r.stderr.count("\n") == 1, (args, r.stderr)
        assert not os.path.exists(tmp_path / "out.pfm")


def test_plane_single_needs_a_medium(built, tmp_path):
    for medium in ((), ("-m", "0.0"), ("-m", "0:0")):
        r = _cli(tmp_path, "plane-single", medium=medium)
        assert r.returncode == 2 and "medium" in r.stderr and r.stderr.count("\n") == 1, (medium, r.stderr)
        assert not os.path.exists(tmp_path / "out.pfm")


def test_unknown_subcommand_lists_plane_single(built, tmp_path):
    r = _cli(tmp_path, "uncorrelated-plane-single")
    assert r.returncode == 2 and "`plane-single`" in r.stderr and r.stderr.count("\n") == 1, r.stderr


def test_plane_single_options_parse_up_to_the_device(built, tmp_path):
    """Well-formed lines (the defaults, every strategy, both spellings of the options) get as far as opening a device: without one, the no-fallback refusal."""
    lines = [("plane-single",), ("plane-single", "--nb-primitive", "16", "--strategy", "cmis")]
    lines += [("plane-single", "-n", "8", "-s", s) for s in api.PLANE_STRATEGIES]
    for args in lines:
        r = _cli(tmp_path, *args)
        if r.returncode == 0:                                  # a machine with a GPU renders it
            assert os.path.exists(tmp_path / "out.pfm")
            os.remove(tmp_path / "out.pfm")
        else:
            assert r.returncode != 2 and "no CPU fallback" in r.stderr, (args, r.stderr)
