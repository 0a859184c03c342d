"""Light-path generation on per-path streams (rl_vpl_generate_paths, kernels/vpl_paths.hip.h) held bit for bit to its restatement from the oracle's entry
points (tests/vpl_paths_restatement.py): the record words, K, the sampler state after and every counter, over the fixtures of
tests/test_vpl_paths_restatement.py, a scene without a medium, Henyey-Greenstein, both seed variants, the streamed BVH and the run-time BSDF switch / a smooth
BSDF; independence of the batch size and of the run; the gather passes downstream of a per-path set; the Python and C++ mirrors and the CLI; the refusals of
rl_vpl_generate with the same codes.  One process; only the CLI test starts a child."""
import os
import subprocess

import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import cli
from tests import bre_restatement as B
from tests import vpl_paths_restatement as R
from tests.scene_helpers import context as _context
from tests.test_gpu_vpl_exact import _scene

pytestmark = pytest.mark.gpu

RL_ERR_INVALID_ARGUMENT = -1
GEN_KEYS = ("camera_samples", "vertices", "extension_rays", "rng_draws")


def _generate(ctx, seed, nb, max_depth=None, rr_depth=0, option=api.VPL_ALL, variant=0):
    sampler = api.IndependentSampler(seed, variant)
    vpls, st = ctx.vpl_generate(sampler, nb, max_depth, rr_depth, option, streams="per_path")
    return vpls, st, sampler


def _check(ctx, ref, seed, nb, max_depth=None, rr_depth=0, option=api.VPL_ALL, variant=0):
    """One generation on the GPU against the restatement's result `ref`: words, K, sampler state, counters.  Returns (set, stats, sampler)."""
    vpls, st, sampler = _generate(ctx, seed, nb, max_depth, rr_depth, option, variant)
    words = vpls.words()
    print("records", words.shape[0], ref["records"].shape[0], "K", vpls.info()[1], ref["n_paths"], "rounds", st["iterations"], "walked", st["paths_walked"])
    np.testing.assert_array_equal(words, ref["records"])
    assert vpls.info() == (ref["records"].shape[0], ref["n_paths"]) and words.shape[0] >= nb
    np.testing.assert_array_equal(np.array(list(sampler.s.s), np.uint64), ref["state"])
    for k in GEN_KEYS:
        assert st[k] == ref["gen_stats"][k], (k, st[k], ref["gen_stats"][k])
    assert st["iterations"] >= 1 and st["kernel_launches"] == st["iterations"] + 1 and st["paths_walked"] >= ref["n_paths"]
    return vpls, st, sampler


def _exact(sd, seed=3, nb=64, max_depth=None, rr_depth=0, option=api.VPL_ALL, variant=0, streaming=False):
    ref = R.compute(sd, seed, nb, max_depth, rr_depth, option, variant)
    return _check(_context(sd, streaming), ref, seed, nb, max_depth, rr_depth, option, variant) + (ref,)


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_fixtures_match_restatement(built, name):
    sd, ref = R.fixture(name)
    _, nb, option, max_depth, rr_depth = R.FIXTURES[name]
    _check(_context(sd), ref, R.FIXTURE_SEED, nb, max_depth, rr_depth, option)


def test_scene_without_a_medium(built):
    _exact(scenes.cbox(32, 24), nb=200)


def test_henyey_greenstein(built):
    _exact(scenes.cbox_medium(32, 24, 1.0, g=0.6), nb=200, option=api.VPL_VOLUME)


@pytest.mark.parametrize("variant", [0, 1])
def test_seed_variants(built, variant):
    _exact(scenes.cbox_medium(24, 16, 1.0), seed=11, nb=120, option=api.VPL_ALL, variant=variant)


@pytest.mark.parametrize("medium", [False, True])
def test_streamed_bvh(built, medium):
    sd = scenes.cbox_medium(24, 16, 1.0) if medium else scenes.cbox(24, 16)
    _exact(sd, seed=7, nb=150, streaming=True)


@pytest.mark.parametrize("name", ["mixed", "glass_and_mirror", "glass"])
def test_bsdf_switch_and_smooth_bsdf(built, name):
    """mixed / glass_and_mirror: MAT = -1, the run-time switch per vertex; glass: one smooth BSDF, only the emitter records are stored."""
    vpls, _, _, _ = _exact(_scene(name), seed=3 if name != "glass" else 1, nb=48, max_depth=6 if name == "glass" else None)
    if name == "glass":
        assert set(np.unique(vpls.records()["kind"])) == {2}


def test_batch_size_changes_nothing(built):
    """vpl_batch_paths = 7: ten rounds and a cut inside a batch; 64: two rounds; unset: the default sizing, one round."""
    sd, ref = R.fixture("depth3")
    _, nb, option, max_depth, rr_depth = R.FIXTURES["depth3"]
    ctx = _context(sd)
    seen = {}
    for batch in (R.FORCED_BATCH, 64, None):
        with ctx.options(vpl_batch_paths=batch):
            vpls, st, sampler = _check(ctx, ref, R.FIXTURE_SEED, nb, max_depth, rr_depth, option)
        seen[batch] = (vpls.words(), vpls.info(), list(sampler.s.s), st)
    rounds7 = -(-ref["n_paths"] // R.FORCED_BATCH)
    assert seen[R.FORCED_BATCH][3]["iterations"] == rounds7 == 10 and seen[R.FORCED_BATCH][3]["paths_walked"] == 7 * rounds7
    assert seen[64][3]["iterations"] == 2 and seen[64][3]["paths_walked"] == 128
    assert seen[None][3]["iterations"] == 1
    for batch in (64, None):
        np.testing.assert_array_equal(seen[batch][0], seen[R.FORCED_BATCH][0])
        assert seen[batch][1:3] == seen[R.FORCED_BATCH][1:3]


def test_default_sizing_takes_a_second_round(built):
    """The many_paths fixture: K lies past the first default batch, so the second batch is sized from the measured records per path."""
    sd, ref = R.fixture("many_paths")
    _, nb, option, _, _ = R.FIXTURES["many_paths"]
    _, st, _ = _check(_context(sd), ref, R.FIXTURE_SEED, nb, option=option)
    assert st["iterations"] == 2 and R.FIRST_DEFAULT_BATCH < ref["n_paths"] <= st["paths_walked"]


def test_lanes_that_walk_several_paths(built):
    """A launch has at most two workgroups per CU (131072 lanes on 256 CUs); a larger batch makes lanes stride over it.  Batches of 65536 paths never stride,
    one of 262144 does, and K is past 131072, so kept paths come from a lane's second turn: the two generations give the same bits.  (GPU against GPU: the
    batches of 65536 are the form the other tests hold to the restatement.)"""
    sd = scenes.cbox_medium(24, 16, 1.0)
    ctx = _context(sd)
    out = []
    for batch in (1 << 16, 1 << 18):
        with ctx.options(vpl_batch_paths=batch):
            vpls, st, sampler = _generate(ctx, 5, 400000, option=api.VPL_SURFACE)
        out.append((vpls.words(), vpls.info(), list(sampler.s.s), {k: st[k] for k in GEN_KEYS}, st["iterations"]))
        vpls.close()
    print("K", out[0][1][1], "records", out[0][1][0], "rounds", out[0][4], out[1][4])
    assert out[0][1][1] > 131072 and out[0][1][0] >= 400000
    assert out[0][4] == -(-out[0][1][1] // (1 << 16)) and out[1][4] == 1
    np.testing.assert_array_equal(out[0][0], out[1][0])
    assert out[0][1:4] == out[1][1:4]


def test_two_calls_from_one_state_give_one_set(built):
    sd, ref = R.fixture("volume")
    _, nb, option, _, _ = R.FIXTURES["volume"]
    ctx = _context(sd)
    a, sta, sa = _generate(ctx, R.FIXTURE_SEED, nb, option=option)
    b, stb, sb = _generate(ctx, R.FIXTURE_SEED, nb, option=option)
    np.testing.assert_array_equal(a.words(), b.words())
    assert a.info() == b.info() and list(sa.s.s) == list(sb.s.s)
    for k in GEN_KEYS + ("iterations", "kernel_launches", "paths_walked"):
        assert sta[k] == stb[k], k


def test_gather_of_a_per_path_set_matches_the_oracle(built):
    """render_vpl on records read back from the GPU, with the block seeds of the advanced sampler."""
    sd, ref = R.fixture("all")
    _, nb, option, _, _ = R.FIXTURES["all"]
    ctx = _context(sd)
    vpls, _, sampler = _check(ctx, ref, R.FIXTURE_SEED, nb, option=option)
    seeds = sampler.block_seeds(sd.width, sd.height)
    np.testing.assert_array_equal(seeds, ref["seeds"])
    img, st = ctx.render_vpl(vpls, seeds, 2)
    want, wst = ref["scene"].render_vpl(vpls.words(), vpls.info()[1], seeds, 2)
    for k in ("camera_samples", "extension_rays", "shadow_rays", "rng_draws", "gather_surface", "gather_volume"):
        assert st[k] == wst[k], (k, st[k], wst[k])
    assert img.any()
    np.testing.assert_array_equal(img, want)


def test_bre_of_a_per_path_set_matches_the_restatement(built):
    sd, ref = R.fixture("volume")
    _, nb, option, _, _ = R.FIXTURES["volume"]
    ctx = _context(sd)
    vpls, _, sampler = _check(ctx, ref, R.FIXTURE_SEED, nb, option=option)
    seeds = sampler.block_seeds(sd.width, sd.height)
    photons = ctx.photon_map(vpls, 0.2)
    img, st = ctx.render_bre(photons, seeds, 2)
    want, wst, _ = B.render(ref["scene"], sd, vpls.words(), vpls.info()[1], seeds, 2, 0.2)
    for k in ("camera_samples", "extension_rays", "rng_draws", "nodes_entered", "photons_gathered"):
        assert st[k] == wst[k], (k, st[k], wst[k])
    assert img.any()
    np.testing.assert_array_equal(img, want)


def test_integrators_compute_the_composition(built):
    sd, ref = R.fixture("all")
    _, nb, option, _, _ = R.FIXTURES["all"]
    integ = api.IntegratorVPL(nb_vpl=nb, option_vpl=option, light_streams="per_path")
    img = integ.compute(api.IndependentSampler(R.FIXTURE_SEED), api.Scene(sd), 2)
    want, _ = ref["scene"].render_vpl(ref["records"], ref["n_paths"], ref["seeds"], 2)
    assert integ.last_generation_stats["camera_samples"] == ref["n_paths"]
    np.testing.assert_array_equal(img, want)
    sd, ref = R.fixture("volume")
    _, nb, _, _, _ = R.FIXTURES["volume"]
    integ = api.IntegratorVolPrimitives(nb_primitive=nb, radius=0.2, light_streams="per_path")
    img = integ.compute(api.IndependentSampler(R.FIXTURE_SEED), api.Scene(sd), 2)
    want, _, _ = B.render(ref["scene"], sd, ref["records"], ref["n_paths"], ref["seeds"], 2, 0.2)
    assert integ.last_generation_stats["camera_samples"] == ref["n_paths"] and img.any()
    np.testing.assert_array_equal(img, want)


def test_cli_writes_what_the_api_renders(built, tmp_path):
    """Both subcommands go through the C++ mirror (integrator.hpp: light_streams = LightStreams::PerPath): the same bytes as the Python mirror, and not the
    serial mode's."""
    scn = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "cbox.pbrt")
    out = str(tmp_path / "out.pfm")
    r = subprocess.run([cli.EXE, scn, "-n", "2", "-r", "independent:7", "-o", out, "vpl", "--nb-vpl", "48", "--light-streams", "per-path"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img = api.load_pfm(out)
    want = api.IntegratorVPL(nb_vpl=48, light_streams="per_path").compute(api.IndependentSampler(7), api.Scene.load(scn), 2)
    serial = api.IntegratorVPL(nb_vpl=48).compute(api.IndependentSampler(7), api.Scene.load(scn), 2)
    assert img.shape == want.shape and want.any()
    np.testing.assert_array_equal(img, want)
    assert not np.array_equal(want, serial)
    r = subprocess.run([cli.EXE, scn, "-n", "2", "-r", "independent:7", "-m", "1.0", "-o", out, "vol-primitivies", "--nb-primitive", "200", "--radius", "0.2",
                        "--light-streams", "per-path"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img = api.load_pfm(out)
    scene = api.Scene.load(scn)
    scene.set_medium((0.0,) * 3, (1.0,) * 3)
    want = api.IntegratorVolPrimitives(nb_primitive=200, radius=0.2, light_streams="per_path").compute(api.IndependentSampler(7), scene, 2)
    assert img.shape == want.shape and want.any()
    np.testing.assert_array_equal(img, want)


def test_refused_inputs(built):
    """What rl_vpl_generate refuses (tests/test_gpu_vpl_exact.py, tests/test_gpu_bre_exact.py), with the same codes; nothing runs and the sampler stays."""
    sd = scenes.cbox(16, 16)
    ctx = _context(sd)
    s = api.IndependentSampler(0)
    before = list(s.s.s)
    for kw, code in (({"max_depth": 1}, RL_ERR_INVALID_ARGUMENT), ({"nb_vpl": 0}, RL_ERR_INVALID_ARGUMENT), ({"nb_vpl": (1 << 20) + 1}, RL_ERR_INVALID_ARGUMENT),
                     ({"option_vpl": 3}, RL_ERR_INVALID_ARGUMENT), ({"option_vpl": -1}, RL_ERR_INVALID_ARGUMENT), ({"option_vpl": api.VPL_VOLUME}, api.RL_ERR_UNSUPPORTED)):
        codes = []
        for streams in api.LIGHT_STREAMS:
            with pytest.raises(api.RustlightError) as e:
                ctx.vpl_generate(s, streams=streams, **kw)
            codes.append(e.value.code)
        assert codes == [code, code], (kw, codes)
    assert list(s.s.s) == before
    with pytest.raises(ValueError):
        ctx.vpl_generate(s, streams="per-path")
    dm = _scene("medium", 8, 8)
    dm.lights.append({"type": "directional", "a": (0.0, -1.0, 0.0), "intensity": (1.0, 1.0, 1.0)})
    with pytest.raises(api.RustlightError) as e:
        _context(dm).vpl_generate(api.IndependentSampler(0), 8, streams="per_path")
    assert e.value.code == api.RL_ERR_UNSUPPORTED
    dark = scenes.cbox(8, 8)
    dark.meshes = [m for m in dark.meshes if m.emission is None]
    with pytest.raises(api.RustlightError) as e:
        _context(dark).vpl_generate(api.IndependentSampler(0), 8, streams="per_path")
    assert e.value.code == api.RL_ERR_NO_EMITTER
    env = scenes.cbox_other_lights(8, 8, point=False, directional=False, environment=True, keep_area_light=True)
    codes = []
    for streams in api.LIGHT_STREAMS:
        with pytest.raises(api.RustlightError) as e:
            _context(env).vpl_generate(api.IndependentSampler(0), 8, streams=streams)
        codes.append(e.value.code)
    assert codes == [api.RL_ERR_UNSUPPORTED] * 2
