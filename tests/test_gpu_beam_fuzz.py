"""A fixed-seed list of random photon-beam cases, each held bit for bit to tests/beam_restatement.py: the cases of the differential fuzzer's bre arm
(tests/parity_fuzz.py: draw_gather_case / gather_scene — frames from 1 x 1 off the 16-grid, coloured media of either phase function, random smooth and
non-smooth BSDFs, streamed BVHs, depth options, a radius of 0.02 .. 0.5, 1 .. 400 beams, both stream modes of the light pass under random batch sizes, one
shard of 2 - 4) with spp folded into 1 .. 3.  The restatement accepts every case the generator can draw: it asks for finite beams with a non-zero summed
length, which every light path in a medium gives (a free path is -ln(1 - u) / sigma_t with u < 1 and sigma_t >= 0.1), and tests/test_beam_restatement.py runs
it on the CPU over beams of the same ranges.  No case is skipped.  One process, no child."""
import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api
from tests import beam_restatement as R
from tests.parity_fuzz import draw_gather_case, gather_scene
from tests.scene_helpers import context as _context

pytestmark = pytest.mark.gpu

N_CASES = 14


def _case(i):
    c = draw_gather_case(np.random.default_rng(7000 + i), "bre")
    c["spp"] = 1 + c["spp"] % 3
    return c


def test_the_list_covers_its_ground():
    """Of the fixed cases: both stream modes, both BVH forms, both phase functions, smooth BSDFs, a shard, every spp, a frame off the 16-grid."""
    cs = [_case(i) for i in range(N_CASES)]
    assert {c["per_path"] for c in cs} == {False, True} and {c["streaming"] for c in cs} == {False, True}
    assert {c["medium"]["hg"] for c in cs} == {False, True} and any(c["bsdfs"] for c in cs) and any(c["shard_count"] > 1 for c in cs)
    assert {c["spp"] for c in cs} == {1, 2, 3} and any(c["size"][0] % 16 and c["size"][1] % 16 for c in cs)
    assert any(c["max_depth"] is None for c in cs) and any(c["max_depth"] is not None for c in cs)


@pytest.mark.parametrize("i", range(N_CASES))
def test_random_case(built, i):
    c = _case(i)
    sd = gather_scene(c)
    ctx, sc = _context(sd, c["streaming"]), orc.Scene(sd)
    sampler = api.IndependentSampler(c["seed"], c["seed_variant"])
    with ctx.options(vpl_batch_paths=c["vpl_batch_paths"]):
        beams, _ = ctx.beam_generate(sampler, c["nb_primitive"], c["max_depth"], c["rr_depth"], "per_path" if c["per_path"] else "reference")
    words, n_paths = beams.words(), beams.info()[1]
    bmap = ctx.beam_map(beams, c["radius"])
    seeds = sampler.block_seeds(*c["size"])
    shard = (c["shard_index"], c["shard_count"])
    img, st = ctx.render_beams(bmap, seeds, c["spp"], c["seed_variant"], *shard)
    ref_img, ref_st, _ = R.render(sc, sd, words, n_paths, seeds, c["spp"], c["radius"], c["seed_variant"], *shard)
    np.testing.assert_array_equal(img, ref_img, err_msg=str(c))
    for k in R.KEYS:
        assert st[k] == ref_st[k], (k, c)
