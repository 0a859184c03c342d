"""The fixtures of tests/test_gpu_vpl_paths_exact.py, on the yardstick alone (tests/vpl_paths_restatement.py, no GPU): the conditions the GPU tests lean on are
asserted here before any of them does — the record and path counts of each fixture, a fixture with paths that store nothing whose K is more than two forced
batches and no multiple of the batch, a fixture whose single path overshoots the count — and the restatement's own claims: a path of the serial pass is one
nb_vpl = 1 call, an option's records are a filter of the VPL_ALL records, the sampler leaves advanced by K draws."""
import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api
from tests import vpl_paths_restatement as R


@pytest.mark.parametrize("name,records,paths", [("volume", 302, 39), ("all", 301, 30), ("surface", 301, 111), ("depth3", 100, 69), ("one_path", 36, 1),
                                                 ("many_paths", 12509, 4214)])
def test_fixture_counts(built, name, records, paths):
    _, ref = R.fixture(name)
    nb = R.FIXTURES[name][1]
    assert (ref["records"].shape[0], ref["n_paths"]) == (records, paths)
    per = ref["per_path"][:, 0].astype(np.int64)
    assert per.sum() == records and records >= nb
    assert per[:-1].sum() < nb                         # K is the smallest count that reaches nb: without the last path it is not reached
    assert ref["gen_stats"]["camera_samples"] == paths


def test_depth3_fixture_has_empty_paths_and_cuts_inside_a_forced_batch(built):
    _, ref = R.fixture("depth3")
    per = ref["per_path"][:, 0]
    assert int(np.count_nonzero(per == 0)) >= 1
    assert ref["n_paths"] > 2 * R.FORCED_BATCH and ref["n_paths"] % R.FORCED_BATCH != 0
    assert -(-ref["n_paths"] // R.FORCED_BATCH) == 10   # ten rounds of 7


def test_one_path_fixture_keeps_all_of_its_path(built):
    _, ref = R.fixture("one_path")
    assert ref["n_paths"] == 1 and ref["records"].shape[0] > R.FIXTURES["one_path"][1]


def test_many_paths_fixture_needs_a_second_default_batch(built):
    """Its kept paths lie beyond index 255 (a lane reaches their seeds through rng_advance's table entries, not by stepping alone) and beyond the first default
    batch, whose size for this count is FIRST_DEFAULT_BATCH."""
    _, ref = R.fixture("many_paths")
    assert R.FIXTURES["many_paths"][1] // 8 < R.FIRST_DEFAULT_BATCH < ref["n_paths"]


def test_sampler_leaves_advanced_by_k_draws(built):
    _, ref = R.fixture("volume")
    main = orc.Rng(R.FIXTURE_SEED)
    for _ in range(ref["n_paths"]):
        main.next_u64()
    assert list(main.state) == [int(v) for v in ref["state"]]
    sd, _ = R.fixture("volume")
    np.testing.assert_array_equal(ref["seeds"], R.block_seeds_after(sd, list(main.state)))


def test_options_filter_the_same_paths(built):
    """option_vpl gates stores, never draws: path k of the three fixtures on the 32x24 frame is the same walk, so the VOLUME and SURFACE records of the first
    paths interleave to the ALL records."""
    _, all_ = R.fixture("all")
    _, vol = R.fixture("volume")
    _, surf = R.fixture("surface")
    k = min(all_["n_paths"], vol["n_paths"], surf["n_paths"])
    for key in (1, 2, 3):                                # vertices, extension rays, draws per path
        np.testing.assert_array_equal(all_["per_path"][:k, key], vol["per_path"][:k, key])
        np.testing.assert_array_equal(all_["per_path"][:k, key], surf["per_path"][:k, key])
    np.testing.assert_array_equal(all_["per_path"][:k, 0], vol["per_path"][:k, 0] + surf["per_path"][:k, 0])
    n = int(all_["per_path"][:k, 0].sum())
    rec = all_["records"][:n]
    np.testing.assert_array_equal(R.keep(rec, api.VPL_VOLUME), vol["records"][: int(vol["per_path"][:k, 0].sum())])
    np.testing.assert_array_equal(R.keep(rec, api.VPL_SURFACE), surf["records"][: int(surf["per_path"][:k, 0].sum())])


def test_first_path_is_the_serial_pass_on_the_forked_stream(built):
    """The serial pass started on path 0's stream with the same count reproduces path 0 and then goes on in that stream: its first records are path 0's."""
    sd, ref = R.fixture("one_path")
    r = orc.Rng(orc.Rng(R.FIXTURE_SEED).next_u64(), 0)
    rec, n, _, _ = ref["scene"].vpl_generate(r.state, R.FIXTURES["one_path"][1], None, 0, api.VPL_VOLUME)
    assert n == 1
    np.testing.assert_array_equal(rec, ref["records"])
