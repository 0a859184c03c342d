"""What the tests that run the `rustlight-amd` CLI share: where it is, the scene they give it, one call, and the two outcomes they hold a line to."""
import os
import subprocess

from rustlight_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(os.path.dirname(api.LIB_PATH), "rustlight-amd")
SCENE = os.path.join(ROOT, "data", "cbox.pbrt")


def run_cli(tmp_path, *args, medium=("-m", "1.0"), spp="2", timeout=60):
    """`rustlight-amd SCENE -n spp [medium] -o tmp_path/out.pfm args...`"""
    return subprocess.run([EXE, SCENE, "-n", spp, *medium, "-o", str(tmp_path / "out.pfm"), *args], capture_output=True, text=True, timeout=timeout)


def assert_refused(tmp_path, args, word, **kwargs):
    """An argument error: exit code 2, one line on stderr that holds `word`, no file written."""
    r = run_cli(tmp_path, *args, **kwargs)
    assert r.returncode == 2 and word in r.stderr and r.stderr.count("\n") == 1, (args, r.stderr)
    assert not os.path.exists(tmp_path / "out.pfm")
    return r


def assert_reaches_device(tmp_path, args, **kwargs):
    """A well-formed line gets as far as opening a device: a machine with a GPU renders it, one without refuses loudly, and not as an argument error."""
    r = run_cli(tmp_path, *args, **kwargs)
    if r.returncode == 0:
        assert os.path.exists(tmp_path / "out.pfm")
        os.remove(tmp_path / "out.pfm")
    else:
        assert r.returncode != 2 and "no CPU fallback" in r.stderr, (args, r.stderr)
