"""`rustlight-amd ... light-tracing`: the argument errors the CLI reports before it opens a device (no GPU needed), the header's rl_light_strategy
values against the Python constants, and the new entry point among the library's exports."""
import ctypes
import os
import re
import subprocess

from rustlight_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, "data", "cbox.pbrt")


def _cli(tmp_path, *args):
    exe = os.path.join(os.path.dirname(api.LIB_PATH), "rustlight-amd")
    return subprocess.run([exe, SCENE, "-n", "4", "-o", str(tmp_path / "out.pfm"), *args], capture_output=True, text=True, timeout=60)


def test_light_tracing_argument_errors(built, tmp_path):
    for args, word in ((("-r", "stratified:3", "light-tracing"), "stratified"),
                       (("-r", "stratified", "light-tracing"), "stratified"),
                       (("--stream-mode", "reference", "light-tracing"), "--stream-mode"),
                       (("--numerics", "fast", "light-tracing"), "fast"),
                       (("light-tracing", "-s", "bsdf"), "bsdf"),
                       (("light-tracing", "-s", "emitter"), "emitter")):
        r = _cli(tmp_path, *args)
        assert r.returncode == 2 and word in r.stderr and r.stderr.count("\n") == 1, (args, r.stderr)
        assert not os.path.exists(tmp_path / "out.pfm")
    r = _cli(tmp_path, "light-tracing", "-x")
    assert r.returncode == 2 and "light-tracing option" in r.stderr, r.stderr


def test_light_strategy_constants_match_the_header():
    header = open(os.path.join(ROOT, "include", "rustlight_amd.h")).read()
    enum = re.search(r"typedef enum rl_light_strategy \{([^}]*)\} rl_light_strategy;", header).group(1)
    values = {k: int(v) for k, v in re.findall(r"(RL_LIGHT_\w+)\s*=\s*(\d+)", enum)}
    assert values == {"RL_LIGHT_ALL": 0, "RL_LIGHT_SURFACE": 1, "RL_LIGHT_VOLUME": 2}
    assert (api.LIGHT_ALL, api.LIGHT_SURFACE, api.LIGHT_VOLUME) == (0, 1, 2)
    assert re.search(r"\bint rl_render_light\(rl_context\* ctx, const rl_path_params\* params,", header)


def test_render_light_is_exported(built):
    assert "rl_render_light" in api.PUBLIC_SYMBOLS
    lib = ctypes.CDLL(api.LIB_PATH)
    assert hasattr(lib, "rl_render_light")
