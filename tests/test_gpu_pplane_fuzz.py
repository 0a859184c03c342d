"""A fixed-seed list of random photon-plane cases, each held bit for bit to tests/pplane_restatement.py, modelled on tests/test_gpu_beam_fuzz.py: the cases of
the differential fuzzer's bre arm (tests/parity_fuzz.py: draw_gather_case / gather_scene — frames from 1 x 1 off the 16-grid, coloured media of either phase
function, random smooth and non-smooth BSDFs, streamed BVHs, depth options, a radius of 0.02 .. 0.5, both stream modes of the light pass under random batch
sizes, one shard of 2 - 4) with spp folded into 1 .. 3 and the plane count into 1 .. 200.

What both sides refuse.  The one refusal the generator could draw is a depth limit of 3, under which no plane exists: _case lifts max_depth to 4 (planes from
the first volume vertex only), so the list holds none, which test_the_list_covers_its_ground checks without a GPU.  The restatement refuses nothing else these
cases can produce: it asks for finite records with a non-zero summed beam length, which every light path in a medium gives (a free path is -ln(1 - u) /
sigma_t with u < 1 and sigma_t >= 0.1; every path stores the beam that leaves the light).  test_the_restatement_refuses_at_most_a_tenth_of_the_list runs the
restatement alone, without a GPU, over records of those ranges on every case's own scene, and counts what it refuses.  A case the device refuses is
skipped only if the restatement refuses the same records, and at most a tenth of the list may be; none is.
One process, no child."""
import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api
from tests import pplane_restatement as Q
from tests.parity_fuzz import draw_gather_case, gather_scene
from tests.scene_helpers import context as _context

N_CASES = 14
SKIPPED = []


def _case(i):
    c = draw_gather_case(np.random.default_rng(9000 + i), "bre")
    c["spp"] = 1 + c["spp"] % 3
    c["nb_primitive"] = 1 + c["nb_primitive"] % 200
    if c["max_depth"] is not None:
        c["max_depth"] = max(4, c["max_depth"])
    return c


def test_the_list_covers_its_ground():
    """Of the fixed cases: both stream modes, both BVH forms, both phase functions, smooth BSDFs, a shard, every spp, a frame off the 16-grid, the smallest
    depth limit; and no case either side refuses for its depth."""
    cs = [_case(i) for i in range(N_CASES)]
    assert {c["per_path"] for c in cs} == {False, True} and {c["streaming"] for c in cs} == {False, True}
    assert {c["medium"]["hg"] for c in cs} == {False, True} and any(c["bsdfs"] for c in cs) and any(c["shard_count"] > 1 for c in cs)
    assert {c["spp"] for c in cs} == {1, 2, 3} and any(c["size"][0] % 16 and c["size"][1] % 16 for c in cs)
    assert any(c["max_depth"] is None for c in cs) and any(c["max_depth"] == 4 for c in cs) and all(c["max_depth"] is None or c["max_depth"] >= 4 for c in cs)


def _records_in_range(c, n_beams=10, n_planes=24):
    """Records with the fields a light path of case c can store: positions in and around the box, unit directions, lengths that are free paths
    -ln(1 - u) / sigma_t of the case's own medium (so finite, and not all zero), positive flux."""
    rs = np.random.default_rng(c["seed"])
    sd = gather_scene(c)
    sigma_t = float(np.min(np.asarray(sd.medium.sigma_a, np.float64) + np.asarray(sd.medium.sigma_s, np.float64)))

    def dirs(n):
        d = rs.normal(size=(n, 3))
        return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)

    def free(n):
        return (-np.log1p(-rs.random(n)) / sigma_t).astype(np.float32)

    def pos(n):
        return rs.uniform((-1.5, -0.5, -1.5), (1.5, 2.5, 6.0), (n, 3)).astype(np.float32)

    beams = Q.R.beam_words(pos(n_beams), free(n_beams), dirs(n_beams), rs.uniform(0.01, 50.0, (n_beams, 3)), rs.random(n_beams) < 0.5, np.arange(n_beams))
    planes = Q.plane_words(pos(n_planes), dirs(n_planes), dirs(n_planes), free(n_planes), free(n_planes), rs.uniform(0.01, 50.0, (n_planes, 3)), np.arange(n_planes) % n_beams, 1)
    return sd, beams, planes


def test_the_restatement_refuses_at_most_a_tenth_of_the_list():
    """Without a GPU: the restatement alone over records of every case's ranges, on the case's own scene, medium, radius and spp (a one-block corner of its frame,
    whole, to keep this quick).  It refuses a case by an AssertionError; the device may skip only those."""
    refused = []
    for i in range(N_CASES):
        c = _case(i)
        sd, beams, planes = _records_in_range(c)
        sd.width, sd.height = min(sd.width, 12), min(sd.height, 9)
        seeds = orc.block_seeds(c["seed"], sd.width, sd.height)
        try:
            img, st, _ = Q.render(orc.Scene(sd), sd, beams, planes, 10, seeds, c["spp"], c["radius"], c["seed_variant"])
        except AssertionError:
            refused.append(i)
            continue
        assert np.isfinite(img).all() and st["camera_samples"] == sd.width * sd.height * c["spp"], c
    assert len(refused) * 10 <= N_CASES, refused


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(N_CASES))
def test_random_case(built, i):
    c = _case(i)
    sd = gather_scene(c)
    ctx, sc = _context(sd, c["streaming"]), orc.Scene(sd)
    sampler = api.IndependentSampler(c["seed"], c["seed_variant"])
    with ctx.options(vpl_batch_paths=c["vpl_batch_paths"]):
        records, _ = ctx.pplane_generate(sampler, c["nb_primitive"], c["max_depth"], c["rr_depth"], "per_path" if c["per_path"] else "reference")
    (planes, beams), n_paths = records.words(), records.info()[2]
    seeds = sampler.block_seeds(*c["size"])
    shard = (c["shard_index"], c["shard_count"])
    try:
        pmap = ctx.pplane_map(records, c["radius"])
    except api.RustlightError:
        with pytest.raises(AssertionError):                       # refused by both, or the case fails
            Q.render(sc, sd, beams, planes, n_paths, seeds, c["spp"], c["radius"], c["seed_variant"], *shard)
        SKIPPED.append(i)
        assert len(SKIPPED) * 10 <= N_CASES, SKIPPED
        pytest.skip("both sides refuse these records")
    img, st = ctx.render_photon_planes(pmap, seeds, c["spp"], c["seed_variant"], *shard)
    ref_img, ref_st, _ = Q.render(sc, sd, beams, planes, n_paths, seeds, c["spp"], c["radius"], c["seed_variant"], *shard)
    np.testing.assert_array_equal(img, ref_img, err_msg=str(c))
    for k in Q.KEYS:
        assert st[k] == ref_st[k], (k, c)
