"""`--light-streams reference|per-path` on `vpl` and `vol-primitivies`: the argument errors the CLI reports before it opens a device (no GPU needed), the lines
that parse, and the declarations of rl_vpl_generate_paths in the header, the ctypes mirror, the Rust block and the option table."""
import os
import re

import pytest

from rustlight_amd import api
from tests import cli
from tests.cli import ROOT


def test_light_streams_argument_errors(built, tmp_path):
    for args, word in ((("vpl", "--light-streams", "per-sample"), "--light-streams"),
                       (("vpl", "--light-streams", "per_path"), "--light-streams"),
                       (("vol-primitivies", "--light-streams", "parallel"), "--light-streams"),
                       (("vol-primitives", "--light-streams", ""), "--light-streams"),
                       (("path", "--light-streams", "per-path"), "--light-streams"),
                       (("ao", "--light-streams", "per-path"), "--light-streams"),
                       (("direct", "--light-streams", "reference"), "--light-streams"),
                       (("light-tracing", "--light-streams", "per-path"), "--light-streams"),
                       (("--light-streams", "per-path", "vpl"), "--light-streams"),
                       # the gather stays in reference order: the camera streams' flag is still refused beside the new one
                       (("--stream-mode", "per-sample", "vpl", "--light-streams", "per-path"), "per-sample"),
                       (("--stream-mode", "per-sample", "vol-primitivies", "--light-streams", "per-path"), "per-sample")):
        cli.assert_refused(tmp_path, args, word)


def test_light_streams_parse_up_to_the_device(built, tmp_path):
    """Well-formed lines get as far as opening a device: without one, the no-fallback refusal."""
    for args in (("vpl", "--light-streams", "per-path", "--nb-vpl", "16"), ("vpl", "--light-streams", "reference", "--nb-vpl", "16"),
                 ("vol-primitivies", "--light-streams", "per-path", "--nb-primitive", "64", "--radius", "0.2"),
                 ("vol-primitives", "--nb-primitive", "64", "--radius", "0.2", "--light-streams", "reference")):
        cli.assert_reaches_device(tmp_path, args)


def test_python_mirrors_take_only_the_two_values():
    assert api.LIGHT_STREAMS == ("reference", "per_path")
    assert api.IntegratorVPL().light_streams == "reference" and api.IntegratorVolPrimitives().light_streams == "reference"
    assert api.IntegratorVPL(light_streams="per_path").light_streams == "per_path"
    assert api.IntegratorVolPrimitives(light_streams="per_path").light_streams == "per_path"
    for cls in (api.IntegratorVPL, api.IntegratorVolPrimitives):
        with pytest.raises(ValueError):
            cls(light_streams="per-sample")


def test_entry_point_is_declared_everywhere(built):
    header = open(os.path.join(ROOT, "include", "rustlight_amd.h")).read()
    m = re.search(r"int rl_vpl_generate_paths\(([^;]*)\);", header)
    g = re.search(r"int rl_vpl_generate\(([^;]*)\);", header)
    assert m and g and " ".join(m.group(1).split()) == " ".join(g.group(1).split())          # rl_vpl_generate's signature
    assert "rl_vpl_generate_paths" in api.PUBLIC_SYMBOLS
    L = api.lib()
    assert L.rl_vpl_generate_paths.argtypes == L.rl_vpl_generate.argtypes
    rust = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"pub fn rl_vpl_generate_paths\(", rust)
    assert "vpl_batch_paths" in header
    knobs = open(os.path.join(ROOT, "rustlight_amd", "csrc", "kernels", "knobs.h")).read()
    assert "K_VPL_BATCH_PATHS" in knobs and '"vpl_batch_paths"' in knobs
    mirror = open(os.path.join(ROOT, "rustlight_amd", "csrc", "host", "integrator.hpp")).read()
    assert mirror.count("LightStreams light_streams = LightStreams::Reference;") == 2
