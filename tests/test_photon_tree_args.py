"""`vol-primitivies --tree-build host|device` and the device build's entry points: the argument errors the CLI reports before it opens a device (no GPU
needed), the lines that parse, and the declarations of rl_photon_map_build_device, rl_photon_tree_build_device and rl_photon_map_read in the header, the
ctypes mirror, the Rust block, the option table and the C++ mirror."""
import os
import re

import pytest

from rustlight_amd import api
from tests import cli
from tests.cli import ROOT

NEW = ("rl_photon_map_build_device", "rl_photon_tree_build_device", "rl_photon_map_read")


def test_tree_build_argument_errors(built, tmp_path):
    for args in (("vol-primitivies", "--tree-build", "bogus"), ("vol-primitives", "--tree-build", ""), ("vol-primitivies", "--tree-build", "gpu"),
                 ("--tree-build", "device", "vol-primitivies"),
                 ("vpl", "--tree-build", "device"), ("path", "--tree-build", "device"), ("ao", "--tree-build", "host"),
                 ("direct", "--tree-build", "device"), ("light-tracing", "--tree-build", "device")):
        cli.assert_refused(tmp_path, args, "--tree-build")


def test_tree_build_parses_up_to_the_device(built, tmp_path):
    """Well-formed lines get as far as opening a device: without one, the no-fallback refusal."""
    for args in (("vol-primitivies", "--tree-build", "device", "--nb-primitive", "64", "--radius", "0.2"),
                 ("vol-primitives", "--nb-primitive", "64", "--radius", "0.2", "--light-streams", "per-path", "--tree-build", "host")):
        cli.assert_reaches_device(tmp_path, args)


def test_python_mirrors_take_only_the_two_values():
    assert api.TREE_BUILDS == ("host", "device")
    assert api.IntegratorVolPrimitives().tree_build == "host"
    assert api.IntegratorVolPrimitives(tree_build="device").tree_build == "device"
    with pytest.raises(ValueError):
        api.IntegratorVolPrimitives(tree_build="gpu")
    ctx = object.__new__(api.Context)                          # the value is refused before the context or the set is touched
    with pytest.raises(ValueError):
        api.Context.photon_map(ctx, None, 0.2, build="x")


def test_entry_points_are_declared_everywhere(built):
    header = open(os.path.join(ROOT, "include", "rustlight_amd.h")).read()
    rust = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = api.lib()
    for name in NEW:
        assert re.search(r"int " + name + r"\(([^;]*)\);", header), name
        assert name in api.PUBLIC_SYMBOLS and getattr(L, name).argtypes is not None, name
        assert re.search(r"pub fn " + name + r"\(", rust), name
    host = " ".join(re.search(r"int rl_photon_tree_build\(([^;]*)\);", header).group(1).split())
    dev = " ".join(re.search(r"int rl_photon_tree_build_device\(([^;]*)\);", header).group(1).split())
    assert dev == "rl_context* ctx, " + host                   # rl_photon_tree_build's contract behind a context
    assert L.rl_photon_tree_build_device.argtypes[1:] == L.rl_photon_tree_build.argtypes
    assert L.rl_photon_map_build_device.argtypes[:4] == L.rl_photon_map_build.argtypes
    m = re.search(r"RL_PHOTON_TREE_GROUP_PHOTONS = (\d+)", header)
    assert m and int(m.group(1)) == api.PHOTON_TREE_GROUP_PHOTONS
    assert "photon_tree_group_photons" in header
    knobs = open(os.path.join(ROOT, "rustlight_amd", "csrc", "kernels", "knobs.h")).read()
    assert "K_PHOTON_TREE_GROUP_PHOTONS" in knobs and '"photon_tree_group_photons"' in knobs
    mirror = open(os.path.join(ROOT, "rustlight_amd", "csrc", "host", "integrator.hpp")).read()
    assert mirror.count("TreeBuild tree_build = TreeBuild::Host;") == 1
