"""`rustlight-amd ... vpl`: the argument errors the CLI reports before it opens a device (no GPU needed) and the parsing of --nb-vpl."""
import os
import subprocess

from rustlight_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, "data", "cbox.pbrt")


def _cli(tmp_path, *args):
    exe = os.path.join(os.path.dirname(api.LIB_PATH), "rustlight-amd")
    return subprocess.run([exe, SCENE, "-n", "4", "-o", str(tmp_path / "out.pfm"), *args], capture_output=True, text=True, timeout=60)


def test_vpl_argument_errors(built, tmp_path):
    for args, word in ((("vpl", "-n", "16"), "--nb-vpl"),
                       (("vpl", "-l", "bsdf"), "-l"),
                       (("vpl", "-v", "emitter"), "-v"),
                       (("-r", "stratified:3", "vpl"), "stratified"),
                       (("--stream-mode", "per-sample", "vpl"), "per-sample"),
                       (("--numerics", "fast", "vpl"), "fast"),
                       (("--gpus", "2", "vpl"), "--gpus"),
                       (("-a", "3", "vpl"), "-a"),
                       (("--frames-in-flight", "2", "vpl"), "--frames-in-flight"),
                       (("vpl", "--nb-vpl", "0"), "--nb-vpl"),
                       (("vpl", "--nb-vpl", "12x"), "--nb-vpl"),
                       (("vpl", "--nb-vpl", str(1 << 21)), "--nb-vpl"),
                       (("vpl", "-s", "all"), "vpl option")):
        r = _cli(tmp_path, *args)
        assert r.returncode == 2 and word in r.stderr and r.stderr.count("\n") == 1, (args, r.stderr)
        assert not os.path.exists(tmp_path / "out.pfm")


def test_vpl_options_parse_up_to_the_device(built, tmp_path):
    """Well-formed `vpl` lines (-b ignored, --nb-vpl, -l / -v, -m / -r with inf) get as far as opening a device: without one, the no-fallback refusal."""
    for args in (("vpl",), ("vpl", "-b", "0.5", "--nb-vpl", "64", "-l", "volume", "-v", "surface", "-m", "6", "-r", "inf"), ("vpl", "-m", "4", "-r", "2")):
        r = _cli(tmp_path, *args)
        if r.returncode == 0:                                  # a machine with a GPU renders it
            assert os.path.exists(tmp_path / "out.pfm")
            os.remove(tmp_path / "out.pfm")
        else:
            assert r.returncode != 2 and "no CPU fallback" in r.stderr, (args, r.stderr)
