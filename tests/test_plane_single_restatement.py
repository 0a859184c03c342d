"""The single-scattering photon planes without a GPU: the host's plane tree (rl_plane_tree_build, csrc/host/planetree.cpp) against the numpy restatement of
BHVAccel::create over SinglePhotonPlane::aabb / position (tests/plane_single_restatement.py) — plane order, node boxes in visiting order, first / count of
every leaf, the skip links, exactly —, the restatement's tree walk against a loop over all planes, DiscreteMIS's three weights at one shared geometry, the
conditions the GPU tests' fixtures have to meet, and the refused inputs."""
import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import plane_single_restatement as R

RL_ERR_INVALID_ARGUMENT = -1


@pytest.fixture(scope="module")
def fixtures(built):
    """cbox_medium(32, 24, 1.0), seed 3, R.FIXTURE_NB planes, spp 2, every strategy: computed once, read by the tests below."""
    sd = scenes.cbox_medium(32, 24, 1.0)
    return {s: R.compute(sd, seed=3, nb_primitive=R.FIXTURE_NB[s], strategy=s, spp=2, want_pairs=(s in ("average", "cmis"))) for s in R.STRATEGIES}


def _same_tree(words):
    boxes, links, order = api.plane_tree_build(words)
    tree = R.build_tree([R.plane_from_words(w) for w in words])
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
    size = {}
    for n in reversed(visit):                          # children come after their parent in visiting order
        node = tree["nodes"][n]
        size[n] = 1 + sum(size[k] for k in (node["left"], node["right"]) if k is not None)
    for i, n in enumerate(visit):                      # a missed box sends the walk to the first node behind the node's subtree
        assert int(links[i, 0]) == i + size[n]
    return tree


@pytest.mark.parametrize("strategy", ["average", "ualpha"])
@pytest.mark.parametrize("n", [1, 4, 5, 9, 64])
def test_tree_of_the_restatements_planes(built, n, strategy):
    """A leaf at the root (1, 4), the 4 / 5 boundary, an odd split, the fixture's size; every plane type (average: UV, VT, UT; ualpha: UAlphaT)."""
    sd = scenes.cbox_medium(32, 24, 1.0)
    _, words, _, _, _, _ = R.generate(sd, list(orc.Rng(n, 0).state), n, strategy)
    tree = _same_tree(words[:n])
    assert (len(tree["nodes"]) == 1) == (n <= 4)


def test_tree_keeps_the_order_of_equal_keys(built):
    """Duplicated planes (their keys tie on every axis): the stable-tie contract."""
    sd = scenes.cbox_medium(32, 24, 1.0)
    planes, words, _, _, _, _ = R.generate(sd, list(orc.Rng(5, 0).state), 6, "average")
    words = np.concatenate([words[:6], words[:6][::-1], words[:6]])
    assert not R.sort_keys_distinct([R.plane_from_words(w) for w in words])
    _same_tree(words)


def test_fixture_conditions(fixtures):
    """Not black against black: every strategy's image is non-zero in at least a quarter of its pixels; planes are intersected, and some are occluded."""
    for s, f in fixtures.items():
        img, st = f["image"], f["stats"]
        lit = np.count_nonzero(img.any(axis=-1))
        print(s, "lit pixels", lit, "of", img.shape[0] * img.shape[1], st)
        assert lit >= 0.25 * img.shape[0] * img.shape[1], s
        assert np.isfinite(img).all(), s
        assert st["planes_intersected"] > st["planes_visible"] > 0, s
        nb = R.FIXTURE_NB[s]
        assert (f["records"].shape[0], f["n_gen"]) == ((66, 22) if s in ("average", "discrete_mis") else (nb, nb))
    d = fixtures["average"]["detail"]
    assert (d["tfar"] < R.F32_MAX).any()
    assert R.sort_keys_distinct(d["planes"])


@pytest.mark.parametrize("strategy", ["average", "cmis"])
def test_tree_walk_against_all_planes(fixtures, strategy):
    """The tree gather and a brute-force pass over all planes give the same (ray, plane) pairs, with the same visibility and the same contributions."""
    d = fixtures[strategy]["detail"]
    brute = R.brute_pairs(d["gatherer"], d["o"], d["d"], d["tfar"])

    def as_dict(pairs):
        out = {}
        for rays, p, vis, val in pairs:
            k = 0
            for r, v in zip(rays, vis):
                out[(int(r), p)] = tuple(val[k]) if v else None
                k += int(v)
        return out
    tree_pairs, all_pairs = as_dict(d["pairs"]), as_dict(brute)
    assert tree_pairs and tree_pairs == all_pairs


def test_discrete_mis_weights_at_one_geometry(built):
    """At one shared geometry (a point, its point on the light, a camera direction) the weights of the UV, UT and VT planes are finite, lie in [0, 1] and, being
    a balance heuristic over the same three terms, sum to 1."""
    sd = scenes.cbox_medium(32, 24, 1.0)
    light = R.rect_lights(sd)[0]
    sigma_s = np.asarray(sd.medium.sigma_s, np.float32)
    rs = np.random.RandomState(11)
    k = 200
    p_light = (light.o[None, :] + light.u[None, :] * (rs.uniform(0, 1, (k, 1)) * light.u_l) + light.v[None, :] * (rs.uniform(0, 1, (k, 1)) * light.v_l)).astype(np.float32)
    p_hit = (p_light + np.asarray([0.0, -1.0, 0.0]) * rs.uniform(0.05, 1.5, (k, 1)) + rs.uniform(-0.3, 0.3, (k, 3))).astype(np.float32)
    rd = rs.normal(size=(k, 3)).astype(np.float32)
    rd = (rd / np.linalg.norm(rd, axis=1, keepdims=True)).astype(np.float32)
    ws = []
    for t in (R.UV, R.UT, R.VT):
        pl = R.Plane()
        pl.type = t
        w = R.discrete_mis_weights(pl, light, sigma_s, p_hit, p_light, rd)
        assert np.isfinite(w).all() and (w >= 0.0).all() and (w <= 1.0).all(), t
        ws.append(w.astype(np.float64))
    np.testing.assert_allclose(ws[0] + ws[1] + ws[2], 1.0, rtol=0, atol=4 * np.finfo(np.float32).eps)      # three roundings of a quotient of f32 sums


def test_generation_counts(built):
    sd = scenes.cbox_medium(32, 24, 1.0)
    for s in R.STRATEGIES:
        planes, words, n_gen, _, draws, redraws = R.generate(sd, list(orc.Rng(3, 0).state), 7, s)
        three = s in ("average", "discrete_mis")
        assert (len(planes), n_gen) == ((9, 3) if three else (7, 7))
        assert draws == n_gen + 6 * len(planes) + 2 * redraws
        want = {"uv": {R.UV}, "vt": {R.VT}, "ut": {R.UT}, "ualpha": {R.UALPHAT}, "cmis": {R.UALPHAT}}.get(s, {R.UV, R.VT, R.UT})
        assert set(int(t) for t in words[:, 16]) == want


def test_sampler_state_inversion(built):
    """state_before undoes one next_u64 (the redraw test of the GPU suite builds its sampler with it)."""
    rng = orc.Rng(12345, 0)
    before = list(rng.state)
    rng.next_u64()
    assert R.state_before(list(rng.state)) == before


def test_refused_inputs(built):
    sd = scenes.cbox_medium(32, 24, 1.0)
    _, words, _, _, _, _ = R.generate(sd, list(orc.Rng(0, 0).state), 8, "vt")
    for bad in (float("nan"), float("inf")):
        for k in (1, 4, 7, 9, 10):                     # o, d0, d1, length0, length1: each reaches a corner
            w2 = words.copy()
            w2[5, k] = np.float32(bad).view(np.uint32)
            with pytest.raises(api.RustlightError) as e:
                api.plane_tree_build(w2)
            assert e.value.code == RL_ERR_INVALID_ARGUMENT, (bad, k)
    boxes, links, order = api.plane_tree_build(words[:0])
    assert boxes.shape[0] == 0 and order.shape[0] == 0
    with pytest.raises(ValueError):
        api.IntegratorSinglePlane(strategy="valpha")
    assert api.IntegratorSinglePlane().strategy == "average" and api.IntegratorSinglePlane().nb_primitive == 128
