"""The two facts the device build of the photon tree (kernels/phototree.hip.h) rests on, pinned to the host build on this machine (no GPU needed): the
topology is a function of the photon count alone, and the host's stable sort of a range equals ANY sort by the unique pair (ordered key, place before the
sort).  tests/photon_tree_cases.py builds the tree level by level from exactly these and must give api.photon_tree_build's arrays, bit for bit."""
import numpy as np
import pytest

from rustlight_amd import api
from tests import photon_tree_cases as P

T = api.PHOTON_TREE_GROUP_PHOTONS
SIZES = (1, 4, 5, 8, 9, 17, 100, 300, T - 1, T, T + 1, 2 * T + 1, 4 * T + 3)


def test_closed_form_node_count():
    for m in list(range(0, 4200)) + [T * 4 + 3, (1 << 20) - 1, 1 << 20, (1 << 20) + 4096]:
        assert P.node_count(m) == (P.node_count_recursive(m) if m else 0), m


def test_ordered_key_orders_like_less_than():
    x = np.array([-np.inf, -3.0e38, -1.5, -1.0e-45, -0.0, 0.0, 1.0e-45, 0.5, 2.0, 3.0e38, np.inf], np.float32)
    k = P.sort_key(x).astype(np.int64)
    assert k[4] == k[5]                                         # the two zeros are one key, as `<` sees them
    assert (np.diff(np.delete(k, 4)) > 0).all()


@pytest.mark.parametrize("family", P.FAMILIES)
def test_level_by_level_build_is_the_host_build(built, family):
    for n in SIZES:
        pos = P.positions(family, n)
        want = api.photon_tree_build(P.words_of(pos), P.RADIUS)
        assert want[0].shape[0] == P.node_count(n)
        P.assert_trees_equal(P.levels_build(pos, P.RADIUS, np.random.default_rng(n)), want, f"{family} n={n}")
        if family == "point":
            np.testing.assert_array_equal(want[2], np.arange(n, dtype=np.uint32))       # all ties: nothing moves


def test_every_size_up_to_a_few_hundred(built):
    for n in range(0, 330):
        pos = P.positions("tied", n, seed=1)
        P.assert_trees_equal(P.levels_build(pos, P.RADIUS), api.photon_tree_build(P.words_of(pos), P.RADIUS), f"n={n}")
