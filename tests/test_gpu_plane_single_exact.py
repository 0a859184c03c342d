"""The single-scattering photon planes (rl_plane_generate / rl_plane_map_build / rl_render_plane_single, kernels/plane.hip.h) held bit for bit to the numpy
restatement of the reference's text (tests/plane_single_restatement.py): the plane records, the counts and the advanced sampler of all seven strategies, a
scene with two lights, the redraw loop on a crafted sampler state; then the image (assert_array_equal) and every counter over all seven strategies and, for
average and discrete_mis, a streamed BVH, a ragged frame at spp 1 and 3 with both seed variants, trees of 4 and 5 planes, two lights and two shards.  The
refused inputs return their codes; the Python mirror equals the restatement's compute, and the CLI (which goes through the C++ mirror's
IntegratorSinglePlane::compute) writes the bytes the Python mirror renders.  The step-by-step comparison (_exact) lives in tests/gather_exact.py, shared with
tests/test_gpu_gather_edges.py, and two_lights in tests/scene_helpers.py; the randomized arm of tests/parity_fuzz.py ("plane": every strategy, coloured
media, random BSDFs, two lights, shards of 2-4) runs from here.  One process; only the CLI test starts a child."""
import os
import subprocess

import numpy as np
import pytest

from oracle import orc
from rustlight_amd import abi, api, scenes
from tests import cli
from tests import plane_single_restatement as R
from tests.gather_exact import PLANE_KEYS as KEYS, plane_exact as _exact
from tests.scene_helpers import context as _context, two_lights

pytestmark = pytest.mark.gpu

RL_ERR_INVALID_ARGUMENT = -1


def _set_state(sampler, state):
    for k in range(4):
        sampler.s.s[k] = int(state[k])


def _generation(ctx, sd, strategy, nb, seed=3, seed_variant=0, state=None):
    """rl_plane_generate against the restatement's plane pass: records, counts, the sampler it leaves, the block seeds.  Returns (PlaneSet, sampler, ref)."""
    if state is None:
        state = list(orc.Rng(seed, seed_variant).state)
    planes, words, n_gen, after, draws, redraws = R.generate(sd, state, nb, strategy)
    sampler = api.IndependentSampler(seed, seed_variant)
    _set_state(sampler, state)
    pset, gst = ctx.plane_generate(sampler, nb, strategy)
    np.testing.assert_array_equal(pset.words(), words)
    assert pset.info() == (words.shape[0], n_gen, strategy)
    assert list(sampler.s.s) == [int(v) for v in after]
    assert (gst["camera_samples"], gst["vertices"], gst["rng_draws"]) == (n_gen, words.shape[0], draws)
    return pset, sampler, {"words": words, "n_gen": n_gen, "after": after, "redraws": redraws}


# ---- generation
@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_generation_matches_restatement(built, strategy):
    sd = scenes.cbox_medium(32, 24, 1.0)
    ctx = _context(sd)
    for nb in (7, 64):
        pset, sampler, ref = _generation(ctx, sd, strategy, nb)
        three = strategy in ("average", "discrete_mis")
        assert len(pset) == ((9 if nb == 7 else 66) if three else nb)
        st = np.array([int(v) for v in ref["after"]], np.uint64)
        want = np.zeros(orc.lib().orc_block_count(32, 24), np.uint64)
        orc.lib().orc_generate_block_seeds(abi.u64ptr(st), 32, 24, abi.u64ptr(want))
        np.testing.assert_array_equal(sampler.block_seeds(32, 24), want)


@pytest.mark.parametrize("strategy", ["average", "ualpha"])
def test_generation_with_two_lights(built, strategy):
    sd = two_lights(32, 24)
    pset, _, ref = _generation(_context(sd), sd, strategy, 64)
    assert set(int(v) for v in ref["words"][:, 17]) == {0, 1}          # both id_emitter values occur


@pytest.mark.parametrize("strategy", ["uv", "discrete_mis", "cmis"])
def test_generation_redraws_a_direction_in_the_light_plane(built, strategy):
    """A first hemisphere coordinate of exactly 0.0 gives z == 0 for more than half of the second coordinates (the restatement's cosine_sample_hemisphere says
    so on the CPU, below): the sampler is handed over in a state whose second draw is 0.0 and whose third gives such a direction, so the first plane's direction
    is drawn again."""
    s1, s2 = 10123822223749065263, 13192915183495924928                # found by search: from (0, s1, s2, 0) the draws are 0.0, 0.6669248938560486
    probe = orc.Rng.from_state([0, s1, s2, 0])
    ux, uy = probe.next_f32(), probe.next_f32()
    assert ux == 0.0 and R.cosine_sample_hemisphere(ux, uy)[2] == 0.0
    state = R.state_before([0, s1, s2, 0])                              # one draw earlier: id_emitter takes the first draw
    sd = scenes.cbox_medium(32, 24, 1.0)
    _, _, ref = _generation(_context(sd), sd, strategy, 7, state=state)
    assert ref["redraws"] >= 1


# ---- image and every counter
@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_every_strategy_matches_restatement(built, strategy):
    """The fixtures of tests/test_plane_single_restatement.py (LDS-staged scene), which asserts on the CPU that each is non-zero in a quarter of its pixels."""
    img, st, _ = _exact(scenes.cbox_medium(32, 24, 1.0), strategy, R.FIXTURE_NB[strategy])
    assert np.count_nonzero(img.any(axis=-1)) >= 0.25 * 32 * 24 and st["planes_intersected"] > 0 and st["planes_visible"] > 0


@pytest.mark.parametrize("strategy", ["average", "discrete_mis"])
def test_streamed_bvh_matches_restatement(built, strategy):
    _exact(scenes.cbox_medium(32, 24, 1.0), strategy, 64, streaming=True)


@pytest.mark.parametrize("strategy", ["average", "discrete_mis"])
@pytest.mark.parametrize("spp,variant", [(1, 0), (1, 1), (3, 0), (3, 1)])
def test_ragged_frame_spp_and_seed_variants(built, strategy, spp, variant):
    _exact(scenes.cbox_medium(40, 24, 1.0), strategy, 64, seed=11, spp=spp, seed_variant=variant)


@pytest.mark.parametrize("strategy,nb", [("ut", 4), ("ut", 5), ("average", 3), ("average", 4), ("average", 5), ("discrete_mis", 3), ("discrete_mis", 4),
                                         ("discrete_mis", 5)])
def test_few_planes(built, strategy, nb):
    """4 planes: the root is a leaf; 5 planes: one split.  average / discrete_mis store three planes per iteration, so asking for 4 or 5 gives 6 (one split)
    and their root is a leaf when 3 are asked for; ut stores exactly what is asked for."""
    _, st, ref = _exact(scenes.cbox_medium(24, 16, 1.0), strategy, nb, seed=1)
    n = ref["records"].shape[0]
    assert n == (nb if strategy == "ut" else 3 * ((nb + 2) // 3))
    assert len(ref["detail"]["tree"]["nodes"]) == (1 if n <= 4 else 3)
    assert st["planes_intersected"] > 0


@pytest.mark.parametrize("strategy", ["average", "discrete_mis"])
def test_two_lights_match_restatement(built, strategy):
    img, st, ref = _exact(two_lights(32, 24), strategy, 64)
    assert set(int(v) for v in ref["records"][:, 17]) == {0, 1} and img.any() and st["planes_visible"] > 0


@pytest.mark.parametrize("strategy", ["average", "discrete_mis"])
def test_two_shards_sum_to_the_frame(built, strategy):
    sd = scenes.cbox_medium(40, 40, 1.0)
    ctx = _context(sd)
    sampler = api.IndependentSampler(4)
    pset, _ = ctx.plane_generate(sampler, 64, strategy)
    pmap = ctx.plane_map(pset)
    seeds = sampler.block_seeds(sd.width, sd.height)
    whole, st = ctx.render_plane_single(pmap, seeds, 2)
    parts = [ctx.render_plane_single(pmap, seeds, 2, shard_index=k, shard_count=2) for k in range(2)]
    assert whole.any()
    np.testing.assert_array_equal(parts[0][0] + parts[1][0], whole)
    assert not np.logical_and(parts[0][0].any(axis=-1), parts[1][0].any(axis=-1)).any()
    for k in KEYS:
        assert parts[0][1][k] + parts[1][1][k] == st[k], k
    sc = orc.Scene(sd)
    words, n_gen = pset.words(), pset.info()[1]
    for k in range(2):                                # each shard against the restatement of that shard
        ref_img, ref_st, _ = R.render(sc, sd, words, n_gen, strategy, seeds, 2, 0, k, 2)
        np.testing.assert_array_equal(parts[k][0], ref_img)
        for key in KEYS:
            assert parts[k][1][key] == ref_st[key], (k, key)


def test_map_read_is_the_host_tree(built):
    sd = scenes.cbox_medium(24, 16, 1.0)
    ctx = _context(sd)
    pset, _ = ctx.plane_generate(api.IndependentSampler(2), 33, "average")
    words = pset.words()
    boxes, links, planes = ctx.plane_map(pset).read()
    want_boxes, want_links, order = api.plane_tree_build(words)
    np.testing.assert_array_equal(boxes, want_boxes)
    np.testing.assert_array_equal(links, want_links)
    w = words[order]
    np.testing.assert_array_equal(planes.view(np.uint32)[:, [0, 1, 2, 4, 5, 6, 8, 9, 10, 3, 7, 12, 13, 14]], w[:, :14])      # o, d0, d1, length0, length1, weight
    np.testing.assert_array_equal(planes.view(np.uint32)[:, 11], w[:, 16] + 4 * w[:, 17])


def test_randomized_plane_parity(built):
    """A short run of the differential fuzzer's plane arm (tests/parity_fuzz.py): every strategy on random frames from 1x1, coloured media, random BSDFs, streamed BVHs, a
    second light, one shard of 2-4; a case both sides refuse (non-finite plane corners) is skipped, and at most a tenth may be."""
    from tests.parity_fuzz import run
    n, bad = run(budget=15.0, seed=22, arm="plane")
    assert bad == 0 and n >= 20, (n, bad)


# ---- refusals
def _code(fn, *a, **kw):
    with pytest.raises(api.RustlightError) as e:
        fn(*a, **kw)
    return e.value.code


def test_refused_scenes(built):
    s = api.IndependentSampler(0)
    assert _code(_context(scenes.cbox(16, 16)).plane_generate, s, 8) == api.RL_ERR_UNSUPPORTED                      # no medium
    sd = scenes.cbox_other_lights(16, 16, point=True, directional=False, environment=False, keep_area_light=False)
    sd.medium = scenes.cbox_medium(16, 16, 1.0).medium
    assert _code(_context(sd).plane_generate, s, 8) == api.RL_ERR_NO_EMITTER                                          # no light mesh (the point light is ignored)
    sd = scenes.cbox_medium(16, 16, 1.0)
    sd.meshes[5].emission = (1.0, 1.0, 1.0)                                                                            # the short box: 12 triangles
    assert _code(_context(sd).plane_generate, s, 8) == api.RL_ERR_UNSUPPORTED
    sd = scenes.cbox_medium(16, 16, 1.0)
    sd.meshes[-1].indices = sd.meshes[-1].indices[:1]                                                                  # one triangle
    assert _code(_context(sd).plane_generate, s, 8) == api.RL_ERR_UNSUPPORTED
    sd = scenes.override_light_emission(scenes.cbox_medium(16, 16, 1.0), "hsv")
    assert _code(_context(sd).plane_generate, s, 8) == api.RL_ERR_UNSUPPORTED
    assert list(s.s.s) == list(api.IndependentSampler(0).s.s)                                                          # nothing was drawn
    # a point light beside the quad is ignored, as the reference ignores it
    sd = scenes.cbox_other_lights(16, 16, point=True, directional=False, environment=False)
    sd.medium = scenes.cbox_medium(16, 16, 1.0).medium
    plain = scenes.cbox_medium(16, 16, 1.0)
    a, _ = _context(sd).plane_generate(api.IndependentSampler(5), 8, "ualpha")
    b, _ = _context(plain).plane_generate(api.IndependentSampler(5), 8, "ualpha")
    np.testing.assert_array_equal(a.words(), b.words())


def test_refused_arguments(built):
    sd = scenes.cbox_medium(16, 16, 1.0)
    ctx, other = _context(sd), _context(sd)
    s = api.IndependentSampler(0)
    for nb in (0, (1 << 20) + 1):
        assert _code(ctx.plane_generate, s, nb) == RL_ERR_INVALID_ARGUMENT, nb
    for strategy in (-1, 7):
        assert _code(ctx.plane_generate, s, 8, strategy) == RL_ERR_INVALID_ARGUMENT, strategy
    pset, _ = ctx.plane_generate(s, 16, "average")
    assert _code(other.plane_map, pset) == RL_ERR_INVALID_ARGUMENT                    # a set from another context
    pmap = ctx.plane_map(pset)
    seeds = s.block_seeds(16, 16)
    assert _code(other.render_plane_single, pmap, seeds) == RL_ERR_INVALID_ARGUMENT   # a map from another context
    for kw, code in (({"spp": (1 << 22) + 1}, api.RL_ERR_UNSUPPORTED), ({"spp": 0}, RL_ERR_INVALID_ARGUMENT),
                     ({"shard_index": 2, "shard_count": 2}, RL_ERR_INVALID_ARGUMENT)):
        assert _code(ctx.render_plane_single, pmap, seeds, **kw) == code, kw


def test_non_finite_corner_is_refused(built):
    """A medium so thin that sampled distances overflow f32: the planes' far corners are not finite.  The restatement says so first."""
    sd = scenes.cbox_medium(16, 16, 1.2e-38)
    state = list(orc.Rng(0, 0).state)
    planes, _, _, _, _, _ = R.generate(sd, state, 512, "ut")
    assert not all(np.isfinite(p.corners()).all() for p in planes)
    s = api.IndependentSampler(0)
    assert _code(_context(sd).plane_generate, s, 512, "ut") == RL_ERR_INVALID_ARGUMENT
    assert list(s.s.s) == state                                                       # the sampler is left as it was


# ---- mirrors
@pytest.mark.parametrize("strategy", ["average", "cmis"])
def test_integrator_compute(built, strategy):
    sd = scenes.cbox_medium(24, 16, 1.0)
    integ = api.IntegratorSinglePlane(nb_primitive=64, strategy=strategy)
    img = integ.compute(api.IndependentSampler(9), api.Scene(sd), 2)
    ref = R.compute(sd, 9, 64, strategy, 2)
    assert img.any()
    np.testing.assert_array_equal(img, ref["image"])


def test_cli_renders_what_the_api_renders(built, tmp_path):
    """`data/cbox.pbrt -m 1.0 -r independent:7 plane-single -n 64 -s cmis` goes through the C++ mirror (integrator.hpp: IntegratorSinglePlane::compute): the
    same bytes as the Python mirror.  The scene file's light is the quad the integrator needs, as it stands."""
    scn = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "cbox.pbrt")
    out = str(tmp_path / "out.pfm")
    r = subprocess.run([cli.EXE, scn, "-n", "2", "-r", "independent:7", "-m", "1.0", "-o", out, "plane-single", "-n", "64", "-s", "cmis"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img = api.load_pfm(out)
    scene = api.Scene.load(scn)
    scene.set_medium((0.0,) * 3, (1.0,) * 3)
    want = api.IntegratorSinglePlane(nb_primitive=64, strategy="cmis").compute(api.IndependentSampler(7), scene, 2)
    assert img.shape == want.shape and want.any()
    np.testing.assert_array_equal(img, want)
