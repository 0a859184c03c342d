"""A fixed-seed list of random virtual-ray-light cases, each held bit for bit to tests/vrl_restatement.py: the cases tests/test_gpu_beam_fuzz.py draws
(tests/parity_fuzz.py: draw_gather_case / gather_scene — frames from 1 x 1 off the 16-grid, coloured media of either phase function, random BSDFs, streamed
BVHs, depth options, a radius of 0.02 .. 0.5, 1 .. 400 beams, both stream modes of the light pass under random batch sizes, one shard of 2 - 4) with spp
folded into 1 .. 3 and other seeds.  The beams that leave a volume vertex are the VRLs: their number, and with it every sample's draw count, follows from the
case.  The restatement accepts every case the generator can draw: a beam pass always stores the light's beam, a surface beam.  No case is skipped; the list as
a whole holds VRLs that pass the roulette and pairs that are visible.  One process, no child."""
import functools

import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api
from tests import vrl_restatement as V
from tests.parity_fuzz import draw_gather_case, gather_scene
from tests.scene_helpers import context as _context

pytestmark = pytest.mark.gpu

N_CASES = 12


def _case(i):
    c = draw_gather_case(np.random.default_rng(9100 + i), "bre")
    c["spp"] = 1 + c["spp"] % 3
    return c


def test_the_list_covers_its_ground():
    cs = [_case(i) for i in range(N_CASES)]
    assert {c["per_path"] for c in cs} == {False, True} and {c["streaming"] for c in cs} == {False, True}
    assert {c["medium"]["hg"] for c in cs} == {False, True} and any(c["shard_count"] > 1 for c in cs)
    assert {c["spp"] for c in cs} == {1, 2, 3} and any(c["size"][0] % 16 and c["size"][1] % 16 for c in cs)
    assert any(c["max_depth"] is None for c in cs) and any(c["max_depth"] is not None for c in cs)


@functools.lru_cache(maxsize=None)
def _run(i):
    """Case i against the restatement, once: (VRLs, accepted, visible)."""
    c = _case(i)
    sd = gather_scene(c)
    ctx, sc = _context(sd, c["streaming"]), orc.Scene(sd)
    sampler = api.IndependentSampler(c["seed"], c["seed_variant"])
    with ctx.options(vpl_batch_paths=c["vpl_batch_paths"]):
        beams, _ = ctx.beam_generate(sampler, c["nb_primitive"], c["max_depth"], c["rr_depth"], "per_path" if c["per_path"] else "reference")
    words, n_paths = beams.words(), beams.info()[1]
    vmap = ctx.vrl_map(beams, c["radius"])
    seeds = sampler.block_seeds(*c["size"])
    shard = (c["shard_index"], c["shard_count"])
    img, st = ctx.render_vrl(vmap, seeds, c["spp"], c["seed_variant"], *shard)
    ref_img, ref_st, _ = V.render(sc, sd, words, n_paths, seeds, c["spp"], c["radius"], c["seed_variant"], *shard)
    for k in V.KEYS:
        assert st[k] == ref_st[k], (k, st[k], ref_st[k], c)
    np.testing.assert_array_equal(img, ref_img, err_msg=str(c))
    return vmap.info()[3], st["vrl_accepted"], st["vrl_visible"]


@pytest.mark.parametrize("i", range(N_CASES))
def test_random_case(built, i):
    _run(i)


def test_the_list_did_not_pass_empty(built):
    """Taken together the cases held VRLs, accepted some and saw some (a case already run is not run again)."""
    seen = np.sum([_run(i) for i in range(N_CASES)], axis=0)
    assert seen[0] > 100 and seen[1] > 100 and seen[2] > 0, seen
