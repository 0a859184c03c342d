"""The device build of the photon tree (rl_photon_map_build_device / rl_photon_tree_build_device, kernels/phototree.hip.h) held to the host build
(rl_photon_tree_build / rl_photon_map_build, which tests/test_bre_restatement.py holds to the reference's text): the tree arrays bit for bit over sizes around
the leaf size and the workgroup's group size T, with the group forced down to 8 and 64 so that a few hundred photons go through five and more global levels,
on random, heavily tied (-0 beside +0) and all-equal positions; the same arrays whatever the group and the run; the host path's refusals; then whole maps,
images and counters from one photon set through both builds, the Python and C++ mirrors and the CLI.  One process; only the CLI test starts a child."""
import functools
import os
import subprocess

import numpy as np
import pytest

from rustlight_amd import api, scenes
from tests import cli
from tests import bre_restatement as R
from tests import photon_tree_cases as P
from tests.scene_helpers import context as _context

pytestmark = pytest.mark.gpu

RL_ERR_INVALID_ARGUMENT = -1
RL_VPL_MAX = 1 << 20
T = api.PHOTON_TREE_GROUP_PHOTONS
KEYS = ("camera_samples", "extension_rays", "rng_draws", "nodes_entered", "photons_gathered")
SIZES = (1, 4, 5, 8, 9, 17, T - 1, T, T + 1, 2 * T + 1, 4 * T + 3)
KNOB = "photon_tree_group_photons"


@functools.lru_cache(maxsize=None)
def _plain_ctx():
    return _context(scenes.cbox(16, 16))                    # the tree entry point needs a device only: no medium here


@functools.lru_cache(maxsize=None)
def _host_tree(family, n):
    return api.photon_tree_build(P.words_of(P.positions(family, n)), P.RADIUS)


@functools.lru_cache(maxsize=None)
def _restatement(g):
    return R.compute(scenes.cbox_medium(32, 24, 1.0, g=g), 3, 300, 3, None, 0, 0.2, 0)


@pytest.mark.parametrize("family", P.FAMILIES)
def test_tree_arrays_equal_the_host_build(built, family):
    ctx = _plain_ctx()
    for n in SIZES:
        got = ctx.photon_tree_build_device(P.words_of(P.positions(family, n)), P.RADIUS)
        P.assert_trees_equal(got, _host_tree(family, n), f"{family} n={n}")
        if family == "point":
            np.testing.assert_array_equal(got[2], np.arange(n, dtype=np.uint32))


@pytest.mark.parametrize("group", [8, 64])
@pytest.mark.parametrize("family", P.FAMILIES)
def test_tree_arrays_through_several_global_levels(built, family, group):
    ctx = _plain_ctx()
    with ctx.options(**{KNOB: group}):
        for n in (9, 17, 100, 300):
            got = ctx.photon_tree_build_device(P.words_of(P.positions(family, n)), P.RADIUS)
            P.assert_trees_equal(got, _host_tree(family, n), f"{family} n={n} group={group}")


def test_nothing_depends_on_the_group_or_the_run(built):
    ctx = _plain_ctx()
    n = 4 * T + 3
    words = P.words_of(P.positions("tied", n))
    want = _host_tree("tied", n)
    for group in (None, None, 8, 64):
        with ctx.options(**{KNOB: group}):
            P.assert_trees_equal(ctx.photon_tree_build_device(words, P.RADIUS), want, f"group={group}")


def test_tree_refusals(built):
    ctx = _plain_ctx()
    n = 2 * T + 1
    pos = P.positions("normal", n)
    for bad in (np.nan, np.inf, -np.inf):
        for rec in (0, n // 2, n - 1):
            p = pos.copy()
            p[rec, rec % 3] = bad
            for fn in (lambda w: api.photon_tree_build(w, P.RADIUS), lambda w: ctx.photon_tree_build_device(w, P.RADIUS)):
                with pytest.raises(api.RustlightError) as e:
                    fn(P.words_of(p))
                assert e.value.code == RL_ERR_INVALID_ARGUMENT and "not finite" in str(e.value), (bad, rec)
    for radius in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(api.RustlightError) as e:
            ctx.photon_tree_build_device(P.words_of(pos[:9]), radius)
        assert e.value.code == RL_ERR_INVALID_ARGUMENT and "radius" in str(e.value), radius
    with pytest.raises(api.RustlightError) as e:
        ctx.photon_tree_build_device(np.zeros((RL_VPL_MAX + 4097, api.VPL_WORDS), np.uint32), P.RADIUS)
    assert e.value.code == RL_ERR_INVALID_ARGUMENT and "too many" in str(e.value)
    P.assert_trees_equal(ctx.photon_tree_build_device(np.zeros((0, api.VPL_WORDS), np.uint32), P.RADIUS),
                         api.photon_tree_build(np.zeros((0, api.VPL_WORDS), np.uint32), P.RADIUS), "no photons")


def _both_maps(ctx, vpls, radius, seeds, spp):
    """Host and device map of one set: read() equal, images equal, counters equal.  Returns the device map's image and counters."""
    host, dev = ctx.photon_map(vpls, radius), ctx.photon_map(vpls, radius, build="device")
    assert host.info() == dev.info()
    assert dev.ms_build > 0.0 and dev.ms_kernels > 0.0 and host.ms_kernels is None
    for name, h, d in zip(("boxes", "links", "photons"), host.read(), dev.read()):
        np.testing.assert_array_equal(d.view(np.uint32), h.view(np.uint32), err_msg=name)
    words = vpls.words()
    boxes, links, order = api.photon_tree_build(words, radius)
    np.testing.assert_array_equal(dev.read()[2].view(np.uint32), words[order, 4:13])      # the photons are the records in leaf order
    img_h, st_h = ctx.render_bre(host, seeds, spp)
    img_d, st_d = ctx.render_bre(dev, seeds, spp)
    for k in KEYS:
        print(k, st_d[k], st_h[k])
    print("pixels that differ:", int(np.count_nonzero((img_d != img_h).any(axis=-1))))
    np.testing.assert_array_equal(img_d, img_h)
    for k in KEYS:
        assert st_d[k] == st_h[k], (k, st_d[k], st_h[k])
    host.close(); dev.close()
    return img_d, st_d


@pytest.mark.parametrize("g", [None, 0.6])
def test_map_and_image_equal_the_host_build_and_the_restatement(built, g):
    sd = scenes.cbox_medium(32, 24, 1.0, g=g)
    ctx = _context(sd)
    sampler = api.IndependentSampler(3)
    vpls, _ = ctx.vpl_generate(sampler, 300, option_vpl=api.VPL_VOLUME)
    seeds = sampler.block_seeds(sd.width, sd.height)
    img, st = _both_maps(ctx, vpls, 0.2, seeds, 3)
    ref = _restatement(g)
    np.testing.assert_array_equal(img, ref["image"])
    for k in KEYS:
        assert st[k] == ref["stats"][k], k
    assert st["photons_gathered"] > 0
    if g is None:
        with ctx.options(**{KNOB: 8}):                       # the same map through six global levels
            img8, _ = _both_maps(ctx, vpls, 0.2, seeds, 3)
        np.testing.assert_array_equal(img8, ref["image"])
        with ctx.options(no_events=1):
            quiet = ctx.photon_map(vpls, 0.2, build="device")
        assert quiet.ms_kernels == 0.0
        quiet.close()


def test_map_of_a_per_path_set(built):
    sd = scenes.cbox_medium(32, 24, 1.0)
    ctx = _context(sd)
    sampler = api.IndependentSampler(3)
    vpls, _ = ctx.vpl_generate(sampler, 300, option_vpl=api.VPL_VOLUME, streams="per_path")
    img, st = _both_maps(ctx, vpls, 0.2, sampler.block_seeds(sd.width, sd.height), 3)
    assert img.any() and st["photons_gathered"] > 0


@pytest.mark.parametrize("nb", [5, 4])
def test_few_photons(built, nb):
    """5 photons: one split; 4 photons: the root is a leaf (the case test_gpu_bre_exact.py pins for the host build)."""
    sd = scenes.cbox_medium(24, 16, 1.0)
    ctx = _context(sd)
    sampler = api.IndependentSampler(1)
    vpls, _ = ctx.vpl_generate(sampler, nb, option_vpl=api.VPL_VOLUME)
    assert vpls.info()[0] == nb
    dev = ctx.photon_map(vpls, 0.5, build="device")
    assert dev.info()[1] == (1 if nb == 4 else 3)
    dev.close()
    _, st = _both_maps(ctx, vpls, 0.5, sampler.block_seeds(sd.width, sd.height), 2)
    assert st["photons_gathered"] > 0


def test_map_refusals(built):
    """The codes tests/test_gpu_bre_exact.py::test_refused_inputs sees from the host path."""
    ctx = _context(scenes.cbox(16, 16))                    # no medium
    surf, _ = ctx.vpl_generate(api.IndependentSampler(0), 8)
    with pytest.raises(api.RustlightError) as e:
        ctx.photon_map(surf, 0.2, build="device")
    assert e.value.code == api.RL_ERR_UNSUPPORTED
    sd = scenes.cbox_medium(16, 16, 1.0)
    ctx = _context(sd)
    s = api.IndependentSampler(0)
    mixed, _ = ctx.vpl_generate(s, 16, option_vpl=api.VPL_ALL)
    messages = []
    for build in api.TREE_BUILDS:
        with pytest.raises(api.RustlightError) as e:
            ctx.photon_map(mixed, 0.2, build=build)        # a set generated with RL_VPL_ALL
        assert e.value.code == RL_ERR_INVALID_ARGUMENT
        messages.append(str(e.value))
    assert messages[0] == messages[1] and "volume records only" in messages[0]
    vol, _ = ctx.vpl_generate(s, 16, option_vpl=api.VPL_VOLUME)
    for radius in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(api.RustlightError) as e:
            ctx.photon_map(vol, radius, build="device")
        assert e.value.code == RL_ERR_INVALID_ARGUMENT, radius
    other = _context(sd)
    with pytest.raises(api.RustlightError) as e:
        other.photon_map(vol, 0.2, build="device")         # a set from another context
    assert e.value.code == RL_ERR_INVALID_ARGUMENT
    photons = ctx.photon_map(vol, 0.2, build="device")
    with pytest.raises(api.RustlightError) as e:
        other.render_bre(photons, s.block_seeds(16, 16))   # a device-built map is a map: another context refuses it all the same
    assert e.value.code == RL_ERR_INVALID_ARGUMENT


def test_integrator_compute(built):
    sd = scenes.cbox_medium(24, 16, 1.0)
    imgs = [api.IntegratorVolPrimitives(nb_primitive=150, radius=0.2, tree_build=b).compute(api.IndependentSampler(9), api.Scene(sd), 2) for b in api.TREE_BUILDS]
    assert imgs[0].any()
    np.testing.assert_array_equal(imgs[1], imgs[0])


def test_cli_writes_the_same_bytes(built, tmp_path):
    """`--tree-build device` goes through the C++ mirror (integrator.hpp: IntegratorVolPrimitives::tree_build): the PFM of the same line without it, byte for byte."""
    scn = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "cbox.pbrt")
    outs = []
    for name, extra in (("host.pfm", []), ("device.pfm", ["--tree-build", "device"])):
        out = str(tmp_path / name)
        r = subprocess.run([cli.EXE, scn, "-n", "2", "-r", "independent:7", "-m", "1.0", "-o", out, "vol-primitivies", "--nb-primitive", "200", "--radius", "0.2", "-n", "3"] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs.append(open(out, "rb").read())
    assert len(outs[0]) > 64 and outs[1] == outs[0]
    assert api.load_pfm(str(tmp_path / "device.pfm")).any()
