"""The uncorrelated photon planes (rl_render_plane_uncorrelated, kernels/uplane.hip.h) held bit for bit to the numpy restatement of the reference's text
(tests/uplane_restatement.py, itself held on the CPU by tests/test_uplane_restatement.py): the image (assert_array_equal) and every counter over all seven
strategies and, for average and discrete_mis, a streamed BVH, a ragged frame at spp 1 and 3 with both seed variants, 1 and 2 planes, two lights, two shards
and frames of 1 x 1 and 1 x 17; a medium so thin that the planes' corners are not finite, which this integrator does not refuse; four block streams in which a
direction is drawn again, so that the lanes behind the redraw start 2 draws later (the kernel's second round).  The refused inputs return their codes; the
Python mirror equals the restatement's compute, and the CLI (the C++ mirror) writes the bytes the Python mirror renders.  One process; only the CLI test
starts a child."""
import os
import subprocess

import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import cli
from tests import uplane_restatement as U
from tests.scene_helpers import context as _context, two_lights

pytestmark = pytest.mark.gpu

RL_ERR_INVALID_ARGUMENT = -1
KEYS = ("camera_samples", "extension_rays", "shadow_rays", "rng_draws", "redraws", "planes_intersected", "planes_visible")


def _same(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    for k in KEYS:
        assert got[1][k] == want[1][k], (k, got[1][k], want[1][k])
    assert got[1]["kernel_launches"] == 1


def _exact(sd, strategy, nb, seed=3, spp=2, seed_variant=0, streaming=False, seeds=None):
    """Render and restatement of one frame, compared: (image, stats, the restatement's detail)."""
    if seeds is None:
        seeds = orc.block_seeds(seed, sd.width, sd.height, seed_variant)
    want = U.render(orc.Scene(sd), sd, seeds, nb, strategy, spp, seed_variant)
    got = _context(sd, streaming).render_plane_uncorrelated(seeds, nb, strategy, spp, seed_variant)
    _same(got, want)
    return got[0], got[1], want[2]


@pytest.mark.parametrize("strategy", U.STRATEGIES)
def test_every_strategy_matches_restatement(built, strategy):
    """The fixtures tests/test_uplane_restatement.py holds to a quarter of lit pixels (LDS-staged scene)."""
    sd, seeds, nb, spp, img, st, _ = U.fixture(strategy)
    got = _context(sd).render_plane_uncorrelated(seeds, nb, strategy, spp)
    _same(got, (img, st))
    assert np.count_nonzero(got[0].any(axis=-1)) >= 0.25 * 32 * 24 and got[1]["planes_visible"] > 0


@pytest.mark.parametrize("strategy", ["average", "discrete_mis"])
def test_streamed_bvh_matches_restatement(built, strategy):
    sd, seeds, nb, spp, img, st, _ = U.fixture(strategy)
    _same(_context(sd, streaming=True).render_plane_uncorrelated(seeds, nb, strategy, spp), (img, st))


@pytest.mark.parametrize("strategy", ["average", "discrete_mis"])
@pytest.mark.parametrize("spp,variant", [(1, 0), (1, 1), (3, 0), (3, 1)])
def test_ragged_frame_spp_and_seed_variants(built, strategy, spp, variant):
    img, _, _ = _exact(scenes.cbox_medium(40, 24, 1.0), strategy, 64, seed=11, spp=spp, seed_variant=variant)
    assert img.any()


@pytest.mark.parametrize("strategy", ["average", "discrete_mis"])
@pytest.mark.parametrize("nb", [1, 2])
def test_one_and_two_planes(built, strategy, nb):
    _, st, _ = _exact(scenes.cbox_medium(32, 24, 1.0), strategy, nb, seed=1, spp=8)
    assert st["rng_draws"] == 32 * 24 * 8 * (2 + 8 * nb) and st["planes_intersected"] > 0


@pytest.mark.parametrize("strategy", ["average", "discrete_mis"])
def test_two_lights_match_restatement(built, strategy):
    img, st, detail = _exact(two_lights(32, 24), strategy, 64)
    assert detail["ids"] == {0, 1} and img.any() and st["planes_visible"] > 0          # both id_emitter values occur


@pytest.mark.parametrize("strategy", ["average", "discrete_mis"])
def test_two_shards_sum_to_the_frame(built, strategy):
    sd = scenes.cbox_medium(40, 40, 1.0)
    ctx = _context(sd)
    seeds = orc.block_seeds(4, 40, 40)
    whole, st = ctx.render_plane_uncorrelated(seeds, 64, strategy, 2)
    parts = [ctx.render_plane_uncorrelated(seeds, 64, strategy, 2, shard_index=k, shard_count=2) for k in range(2)]
    assert whole.any()
    np.testing.assert_array_equal(parts[0][0] + parts[1][0], whole)
    assert not np.logical_and(parts[0][0].any(axis=-1), parts[1][0].any(axis=-1)).any()
    for k in KEYS:
        assert parts[0][1][k] + parts[1][1][k] == st[k], k
    sc = orc.Scene(sd)
    for k in range(2):                                # each shard against the restatement of that shard
        _same(parts[k], U.render(sc, sd, seeds, 64, strategy, 2, 0, k, 2))


@pytest.mark.parametrize("strategy", ["average", "discrete_mis"])
@pytest.mark.parametrize("w,h", [(1, 1), (1, 17)])
def test_smallest_frames(built, strategy, w, h):
    """One lane of one block; one column over two blocks, the second a single lane.  The quarter of lit pixels does not apply: 256 planes at 4 spp so that
    something is lit at all, asserted."""
    img, _, _ = _exact(scenes.cbox_medium(w, h, 1.0), strategy, 256, seed=5, spp=4)
    assert img.any()


def test_thin_medium_is_not_refused(built):
    """sigma_s = 1.2e-38: sampled distances overflow f32 and the planes' far corners are not finite (the restatement says so first).  plane-single refuses such
    a set; here there is no tree to refuse it, and the planes go through the intersection's comparisons as they do in the reference."""
    sd = scenes.cbox_medium(16, 16, 1.2e-38)
    seeds = orc.block_seeds(0, 16, 16)
    want = U.render(orc.Scene(sd), sd, seeds, 64, "ut", 2)
    assert not want[2]["corners_finite"]
    _same(_context(sd).render_plane_uncorrelated(seeds, 64, "ut", 2), want)


@pytest.mark.parametrize("i", range(len(U.REDRAW_CASES)))
def test_a_direction_drawn_again_moves_the_lanes_behind_it(built, i):
    """A block stream with an exact 0.0 where a direction's coordinate is drawn (tests/test_uplane_restatement.py holds lane, sample and plane): the lanes
    behind the redraw run again from 2 draws further on."""
    sd, seeds, block, (seed, strategy, nb, spp, lane, sample, plane), img, st, detail = U.redraw_case(i)
    got = _context(sd).render_plane_uncorrelated(seeds, nb, strategy, spp)
    _same(got, (img, st))
    assert got[1]["redraws"] >= 1
    assert got[1]["rng_draws"] == got[1]["camera_samples"] * U.draws_per_sample(nb, strategy) + 2 * got[1]["redraws"]


# ---- refusals
def _code(fn, *a, **kw):
    with pytest.raises(api.RustlightError) as e:
        fn(*a, **kw)
    return e.value.code


def test_refused_scenes(built):
    seeds = orc.block_seeds(0, 16, 16)
    assert _code(_context(scenes.cbox(16, 16)).render_plane_uncorrelated, seeds, 8) == api.RL_ERR_UNSUPPORTED                   # no medium
    sd = scenes.cbox_other_lights(16, 16, point=True, directional=False, environment=False, keep_area_light=False)
    sd.medium = scenes.cbox_medium(16, 16, 1.0).medium
    assert _code(_context(sd).render_plane_uncorrelated, seeds, 8) == api.RL_ERR_NO_EMITTER                                       # no light mesh
    sd = scenes.cbox_medium(16, 16, 1.0)
    sd.meshes[5].emission = (1.0, 1.0, 1.0)                                                                                        # the short box: 12 triangles
    assert _code(_context(sd).render_plane_uncorrelated, seeds, 8) == api.RL_ERR_UNSUPPORTED
    sd = scenes.cbox_medium(16, 16, 1.0)
    sd.meshes[-1].indices = sd.meshes[-1].indices[:1]                                                                              # one triangle
    assert _code(_context(sd).render_plane_uncorrelated, seeds, 8) == api.RL_ERR_UNSUPPORTED
    sd = scenes.override_light_emission(scenes.cbox_medium(16, 16, 1.0), "hsv")
    assert _code(_context(sd).render_plane_uncorrelated, seeds, 8) == api.RL_ERR_UNSUPPORTED


def test_refused_arguments(built):
    sd = scenes.cbox_medium(16, 16, 1.0)
    ctx = _context(sd)
    seeds = orc.block_seeds(0, 16, 16)
    for nb in (0, (1 << 20) + 1):
        assert _code(ctx.render_plane_uncorrelated, seeds, nb) == RL_ERR_INVALID_ARGUMENT, nb
    for strategy in (-1, 7):
        assert _code(ctx.render_plane_uncorrelated, seeds, 8, strategy) == RL_ERR_INVALID_ARGUMENT, strategy
    for kw, code in (({"spp": 0}, RL_ERR_INVALID_ARGUMENT), ({"shard_index": 2, "shard_count": 2}, RL_ERR_INVALID_ARGUMENT)):
        assert _code(ctx.render_plane_uncorrelated, seeds, 8, **kw) == code, kw
    assert _code(ctx.render_plane_uncorrelated, seeds[:0], 8) == RL_ERR_INVALID_ARGUMENT
    # the jump-ahead's reach, 256 * spp * D <= 2^32 - 1: D = 2 + 7 * 2396 = 16774 at 1000 spp is the last that fits, one plane more is refused before any kernel
    assert 256 * 1000 * (2 + 7 * 2396) <= 2 ** 32 - 1 < 256 * 1000 * (2 + 7 * 2397)
    assert _code(ctx.render_plane_uncorrelated, seeds, 2397, "ut", spp=1000) == api.RL_ERR_UNSUPPORTED
    assert _code(ctx.render_plane_uncorrelated, seeds, 1 << 20, "average", spp=2) == api.RL_ERR_UNSUPPORTED


# ---- mirrors
@pytest.mark.parametrize("strategy", ["average", "cmis"])
def test_integrator_compute(built, strategy):
    sd = scenes.cbox_medium(24, 16, 1.0)
    integ = api.IntegratorSinglePlaneUncorrelated(nb_primitive=64, strategy=strategy)
    img = integ.compute(api.IndependentSampler(9), api.Scene(sd), 2)
    ref = U.compute(sd, 9, 64, strategy, 2)
    assert img.any()
    np.testing.assert_array_equal(img, ref["image"])
    for k in KEYS:
        assert integ.last_stats[k] == ref["stats"][k], k


def test_cli_renders_what_the_api_renders(built, tmp_path):
    """`data/cbox.pbrt -n 2 -m 1.0 -r independent:7 plane-single --uncorrelated -n 64 -s cmis` goes through the C++ mirror (integrator.hpp:
    IntegratorSinglePlaneUncorrelated::compute): the same bytes as the Python mirror."""
    scn = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "cbox.pbrt")
    out = str(tmp_path / "out.pfm")
    r = subprocess.run([cli.EXE, scn, "-n", "2", "-m", "1.0", "-r", "independent:7", "-o", out, "plane-single", "--uncorrelated", "-n", "64", "-s", "cmis"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img = api.load_pfm(out)
    scene = api.Scene.load(scn)
    scene.set_medium((0.0,) * 3, (1.0,) * 3)
    want = api.IntegratorSinglePlaneUncorrelated(nb_primitive=64, strategy="cmis").compute(api.IndependentSampler(7), scene, 2)
    assert img.shape == want.shape and want.any()
    np.testing.assert_array_equal(img, want)
