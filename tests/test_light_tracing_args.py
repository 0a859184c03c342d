"""`rustlight-amd ... light-tracing`: the argument errors the CLI reports before it opens a device (no GPU needed), the header's rl_light_strategy
values against the Python constants, and the new entry point among the library's exports."""
import ctypes
import os
import re

from rustlight_amd import api
from tests import cli
from tests.cli import ROOT

PLAIN = dict(medium=(), spp="4")      # these lines: 4 spp and no medium


def test_light_tracing_argument_errors(built, tmp_path):
    for args, word in ((("-r", "stratified:3", "light-tracing"), "stratified"),
                       (("-r", "stratified", "light-tracing"), "stratified"),
                       (("--stream-mode", "reference", "light-tracing"), "--stream-mode"),
                       (("--numerics", "fast", "light-tracing"), "fast"),
                       (("light-tracing", "-s", "bsdf"), "bsdf"),
                       (("light-tracing", "-s", "emitter"), "emitter")):
        cli.assert_refused(tmp_path, args, word, **PLAIN)
    r = cli.run_cli(tmp_path, "light-tracing", "-x", **PLAIN)
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
