"""The beam radiance estimate (rl_photon_map_build / rl_render_bre, kernels/bre.hip.h) held bit for bit to the numpy restatement of the reference's text
(tests/bre_restatement.py): first the photon records, the path count and the advanced sampler against the oracle's orc_vpl_generate, then the image
(assert_array_equal) and every counter, over both phase functions, LDS-staged and streamed BVHs, a ragged frame, spp 1 and 5, both seed variants, trees whose
root is a leaf, depth options and two shards.  The refused inputs return their codes; the CLI (which goes through the C++ mirror's
IntegratorVolPrimitives::compute) writes the bytes the API renders.  The step-by-step comparison (_exact) lives in tests/gather_exact.py, shared with
tests/test_gpu_gather_edges.py; the randomized arm of tests/parity_fuzz.py ("bre": coloured media, random BSDFs, both tree builds, per-path sets, shards of
2-4) runs from here.  One process; only the CLI test starts a child."""
import os
import subprocess

import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import cli
from tests import bre_restatement as R
from tests.gather_exact import BRE_KEYS as KEYS, bre_exact as _exact
from tests.scene_helpers import context as _context

pytestmark = pytest.mark.gpu

RL_ERR_INVALID_ARGUMENT = -1


@pytest.mark.parametrize("g", [None, 0.6])
def test_fixture_matches_restatement(built, g):
    """The fixture of tests/test_bre_restatement.py (LDS-staged scene); g = 0.6: the Henyey-Greenstein instantiation."""
    img, st, _ = _exact(scenes.cbox_medium(32, 24, 1.0, g=g))
    assert np.count_nonzero(img.any(axis=-1)) >= 0.25 * 32 * 24 and st["photons_gathered"] > 0


def test_streamed_bvh_matches_restatement(built):
    _exact(scenes.cbox_medium(32, 24, 1.0), streaming=True)


@pytest.mark.parametrize("spp,variant", [(1, 0), (1, 1), (5, 0), (5, 1)])
def test_ragged_frame_spp_and_seed_variants(built, spp, variant):
    _exact(scenes.cbox_medium(40, 24, 1.0), seed=11, spp=spp, seed_variant=variant, nb_primitive=120)


@pytest.mark.parametrize("nb,radius", [(5, 0.5), (4, 0.5)])
def test_few_photons(built, nb, radius):
    """5 photons: one split; 4 photons: the root is a leaf.  (With seed 1 the last light path ends exactly on the count.)"""
    _, st, ref = _exact(scenes.cbox_medium(24, 16, 1.0), seed=1, nb_primitive=nb, spp=2, radius=radius)
    assert ref["records"].shape[0] == nb and st["photons_gathered"] > 0
    assert len(ref["detail"]["tree"]["nodes"]) == (1 if nb == 4 else 3)


def test_depth_and_rr_options(built):
    _exact(scenes.cbox_medium(24, 16, 1.0), seed=2, nb_primitive=100, max_depth=3, rr_depth=2)


def test_two_shards_sum_to_the_frame(built):
    sd = scenes.cbox_medium(40, 40, 1.0)
    ctx = _context(sd)
    sampler = api.IndependentSampler(4)
    vpls, _ = ctx.vpl_generate(sampler, 200, option_vpl=api.VPL_VOLUME)
    photons = ctx.photon_map(vpls, 0.2)
    seeds = sampler.block_seeds(sd.width, sd.height)
    whole, st = ctx.render_bre(photons, seeds, 2)
    parts = [ctx.render_bre(photons, seeds, 2, shard_index=k, shard_count=2) for k in range(2)]
    assert whole.any()
    np.testing.assert_array_equal(parts[0][0] + parts[1][0], whole)
    assert not np.logical_and(parts[0][0].any(axis=-1), parts[1][0].any(axis=-1)).any()
    for k in KEYS:
        assert parts[0][1][k] + parts[1][1][k] == st[k], k
    sc = orc.Scene(sd)
    words, n_paths = vpls.words(), vpls.info()[1]
    for k in range(2):                                # each shard against the restatement of that shard
        ref_img, ref_st, _ = R.render(sc, sd, words, n_paths, seeds, 2, 0.2, 0, k, 2)
        np.testing.assert_array_equal(parts[k][0], ref_img)
        for key in KEYS:
            assert parts[k][1][key] == ref_st[key], (k, key)


def test_randomized_bre_parity(built):
    """A short run of the differential fuzzer's bre arm (tests/parity_fuzz.py): random frames from 1x1, coloured media with either phase function, random BSDFs,
    streamed BVHs, depth options, per-path photon sets, the device-built tree under random group sizes (its map equal to the host's array for array), one shard of 2-4."""
    from tests.parity_fuzz import run
    n, bad = run(budget=15.0, seed=21, arm="bre")
    assert bad == 0 and n >= 20, (n, bad)


def test_refused_inputs(built):
    plain = scenes.cbox(16, 16)                       # no medium
    ctx = _context(plain)
    with pytest.raises(api.RustlightError) as e:
        ctx.vpl_generate(api.IndependentSampler(0), 8, option_vpl=api.VPL_VOLUME)
    assert e.value.code == api.RL_ERR_UNSUPPORTED
    surf, _ = ctx.vpl_generate(api.IndependentSampler(0), 8)
    with pytest.raises(api.RustlightError) as e:
        ctx.photon_map(surf, 0.2)
    assert e.value.code == api.RL_ERR_UNSUPPORTED
    sd = scenes.cbox_medium(16, 16, 1.0)
    ctx = _context(sd)
    s = api.IndependentSampler(0)
    mixed, _ = ctx.vpl_generate(s, 16, option_vpl=api.VPL_ALL)
    with pytest.raises(api.RustlightError) as e:
        ctx.photon_map(mixed, 0.2)                    # a set generated with RL_VPL_ALL
    assert e.value.code == RL_ERR_INVALID_ARGUMENT
    vol, _ = ctx.vpl_generate(s, 16, option_vpl=api.VPL_VOLUME)
    for radius in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(api.RustlightError) as e:
            ctx.photon_map(vol, radius)
        assert e.value.code == RL_ERR_INVALID_ARGUMENT, radius
    other = _context(sd)
    with pytest.raises(api.RustlightError) as e:
        other.photon_map(vol, 0.2)                    # a set from another context
    assert e.value.code == RL_ERR_INVALID_ARGUMENT
    photons = ctx.photon_map(vol, 0.2)
    seeds = s.block_seeds(16, 16)
    with pytest.raises(api.RustlightError) as e:
        other.render_bre(photons, seeds)              # a map from another context
    assert e.value.code == RL_ERR_INVALID_ARGUMENT
    for kw, code in (({"spp": (1 << 22) + 1}, api.RL_ERR_UNSUPPORTED), ({"spp": 0}, RL_ERR_INVALID_ARGUMENT),
                     ({"shard_index": 2, "shard_count": 2}, RL_ERR_INVALID_ARGUMENT)):
        with pytest.raises(api.RustlightError) as e:
            ctx.render_bre(photons, seeds, **kw)
        assert e.value.code == code, kw
    with pytest.raises(api.RustlightError) as e:
        ctx.vpl_generate(s, 16, max_depth=1, option_vpl=api.VPL_VOLUME)
    assert e.value.code == RL_ERR_INVALID_ARGUMENT


def test_integrator_compute(built):
    sd = scenes.cbox_medium(24, 16, 1.0)
    integ = api.IntegratorVolPrimitives(nb_primitive=150, radius=0.2)
    img = integ.compute(api.IndependentSampler(9), api.Scene(sd), 2)
    ref = R.compute(sd, 9, 150, 2, radius=0.2)
    assert img.any()
    np.testing.assert_array_equal(img, ref["image"])


def test_cli_renders_what_the_api_renders(built, tmp_path):
    """`vol-primitivies` goes through the C++ mirror (integrator.hpp: IntegratorVolPrimitives::compute): the same bytes as the Python mirror; -p beam is not built."""
    scn = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "cbox.pbrt")
    out = str(tmp_path / "out.pfm")
    args = [cli.EXE, scn, "-n", "2", "-r", "independent:7", "-m", "1.0", "-o", out]
    r = subprocess.run(args + ["vol-primitivies", "--nb-primitive", "200", "--radius", "0.2", "-n", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img = api.load_pfm(out)
    scene = api.Scene.load(scn)
    scene.set_medium((0.0,) * 3, (1.0,) * 3)
    want = api.IntegratorVolPrimitives(nb_primitive=200, radius=0.2).compute(api.IndependentSampler(7), scene, 2)
    assert img.shape == want.shape and want.any()
    np.testing.assert_array_equal(img, want)
    r = subprocess.run(args + ["vol-primitives", "-p", "beam"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "not built" in r.stderr
