"""The beam radiance estimate without a GPU: the host's photon tree (rl_photon_tree_build, csrc/host/photontree.cpp) against the numpy restatement of
BHVAccel::create (tests/bre_restatement.py) — photon order, node boxes in visiting order, first / count of every leaf, exactly —, the restatement's tree walk
against a loop over all photons, the conditions the GPU tests' fixture has to meet, and the refused inputs."""
import numpy as np
import pytest

from rustlight_amd import api, scenes
from tests import bre_restatement as R

RL_ERR_INVALID_ARGUMENT = -1


@pytest.fixture(scope="module")
def fixture(built):
    """cbox_medium(32, 24, 1.0), seed 3, 300 photons, radius 0.2, spp 3: computed once, read by every test below."""
    return R.compute(scenes.cbox_medium(32, 24, 1.0), seed=3, nb_primitive=300, spp=3, radius=0.2, want_pairs=True)


def _words(pos):
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    w = np.zeros((pos.shape[0], api.VPL_WORDS), np.uint32)
    w[:, 0] = 1
    w[:, 4:7] = pos.view(np.uint32)
    return w


def _same_tree(words, radius):
    boxes, links, order = api.photon_tree_build(words, radius)
    tree = R.build_tree(R.records_of(words)[0], radius)
    visit = R.visit_order(tree)
    np.testing.assert_array_equal(order, tree["order"])
    assert boxes.shape[0] == len(visit) == len(tree["nodes"])
    for i, n in enumerate(visit):
        node = tree["nodes"][n]
        np.testing.assert_array_equal(boxes[i], np.concatenate([node["lo"], node["hi"]]))
        leaf = node["left"] is None and node["right"] is None
        assert (int(links[i, 2]) > 0) == leaf
        if leaf:
            assert (int(links[i, 1]), int(links[i, 2])) == (node["first"], node["count"])
    # the skip links: a missed box sends the walk to the first node behind the node's subtree
    size = {}
    for n in reversed(visit):                          # children come after their parent in visiting order
        node = tree["nodes"][n]
        size[n] = 1 + sum(size[k] for k in (node["left"], node["right"]) if k is not None)
    for i, n in enumerate(visit):
        assert int(links[i, 0]) == i + size[n]
    return tree


def test_tree_of_the_fixture(fixture):
    tree = _same_tree(fixture["records"], 0.2)
    assert len(tree["nodes"]) > 64


@pytest.mark.parametrize("n", range(1, 10))
def test_tree_of_few_photons(built, n):
    """A leaf at the root (1-4), the 4 / 5 boundary, odd splits."""
    rs = np.random.RandomState(n)
    tree = _same_tree(_words(rs.uniform(-1, 1, (n, 3))), 0.25)
    assert (len(tree["nodes"]) == 1) == (n <= 4)


def test_tree_keeps_the_order_of_equal_keys(built):
    """Duplicated positions (and -0 beside +0): the stable-tie contract."""
    rs = np.random.RandomState(7)
    base = rs.uniform(-1, 1, (6, 3)).astype(np.float32)
    pos = np.concatenate([base, base[::-1], base, [[0.0, 0.5, 0.5], [-0.0, 0.5, 0.5], [0.0, 0.5, 0.5]]]).astype(np.float32)
    assert not R.sort_keys_distinct(pos)
    _same_tree(_words(pos), 0.1)


def test_fixture_conditions(fixture):
    """Conditions on the input, asserted of the restatement before anything is compared with it."""
    img, d = fixture["image"], fixture["detail"]
    assert fixture["records"].shape[0] >= 300 and (fixture["records"][:, 0] == 1).all()
    assert np.count_nonzero(img.any(axis=-1)) >= 0.25 * img.shape[0] * img.shape[1]
    per_sample = np.zeros(d["d"].shape[0], np.int64)
    for rays, _, _ in d["pairs"]:
        per_sample[rays] += 1
    assert per_sample.max() >= 5
    assert R.sort_keys_distinct(d["photons"].pos)
    assert fixture["stats"]["photons_gathered"] == per_sample.sum()
    assert (d["tfar"] == R.F32_MAX).any() and (d["tfar"] < R.F32_MAX).any()        # rays that leave the scene, and rays that do not


def test_tree_walk_against_all_photons(fixture):
    d = fixture["detail"]
    brute = R.brute_pairs(d["photons"], d["o"], d["d"], d["tfar"])
    n = d["d"].shape[0]
    all_pairs = {(int(r), p) for rays, p, _ in brute for r in rays}
    tree_pairs = {(int(r), p) for rays, p, _ in d["pairs"] for r in rays}
    assert tree_pairs and tree_pairs <= all_pairs
    sums = []
    for pairs in (d["pairs"], brute):
        s = np.zeros((n, 3), np.float64)
        for rays, _, val in pairs:
            s[rays] += val.astype(np.float64)
        sums.append(s)
    np.testing.assert_allclose(sums[0], sums[1], rtol=1e-6, atol=0.0)


def test_refused_inputs(built):
    w = _words(np.random.RandomState(0).uniform(-1, 1, (8, 3)))
    for radius in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(api.RustlightError) as e:
            api.photon_tree_build(w, radius)
        assert e.value.code == RL_ERR_INVALID_ARGUMENT, radius
    for bad in (float("nan"), float("inf")):
        w2 = w.copy()
        w2[5, 5] = np.float32(bad).view(np.uint32)
        with pytest.raises(api.RustlightError) as e:
            api.photon_tree_build(w2, 0.1)
        assert e.value.code == RL_ERR_INVALID_ARGUMENT, bad
    with pytest.raises(api.RustlightError):
        api.IntegratorVolPrimitives(primitives="beam")
