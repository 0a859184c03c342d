"""The photon beams without a GPU: the numpy restatement (tests/beam_restatement.py) against a literal scalar walk of the reference's text and against closed
forms, then the host's split and beam tree (rl_beam_split, rl_beam_tree_build, csrc/host/beamtree.cpp) against the restatement byte for byte, and the refused
inputs.

A note on the sub-beam counts: sum_i ceil(l_i / avg_split) >= sum_i l_i / avg_split = 5 n, so the split of a non-empty set never makes fewer than 5 sub-beams.
Trees of 1 to 4 elements (a leaf at the root) are therefore built here from sub-beam records handed to rl_beam_tree_build directly."""
import math
import types

import numpy as np
import pytest

from rustlight_amd import api
from tests import beam_restatement as R
from tests import bre_restatement as B
from tests.photon_tree_cases import assert_trees_equal

F32 = np.float32
RL_ERR_INVALID_ARGUMENT = -1


def _random_beams(rs, n, zero_every=0):
    o = rs.uniform(-1, 1, (n, 3)).astype(np.float32)
    d = rs.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    length = rs.uniform(0.05, 2.5, n).astype(np.float32)
    if zero_every:
        length[::zero_every] = 0.0
    rad = rs.uniform(0.1, 3.0, (n, 3)).astype(np.float32)
    return R.beam_words(o, length, d, rad, from_surface=rs.uniform(size=n) < 0.5, path=np.arange(n))


def _random_rays(rs, n):
    o = rs.uniform(-1.5, 1.5, (n, 3)).astype(np.float32)
    d = rs.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    tfar = np.where(rs.uniform(size=n) < 0.25, R.F32_MAX, rs.uniform(0.5, 4.0, n)).astype(np.float32)
    return o, d, tfar


def _medium(sigma_a, sigma_s):
    return types.SimpleNamespace(sigma_a=sigma_a, sigma_s=sigma_s, phase=0, g=0.0)


# ---- the reference's text, one scalar float32 operation at a time
def _dot(a, b):
    return F32(F32(F32(a[0] * b[0]) + F32(a[1] * b[1])) + F32(a[2] * b[2]))


def _cross(a, b):
    return np.array([F32(F32(a[1] * b[2]) - F32(a[2] * b[1])), F32(F32(a[2] * b[0]) - F32(a[0] * b[2])), F32(F32(a[0] * b[1]) - F32(a[1] * b[0]))], np.float32)


def _intersection(bo, bd, blen, radius, ro, rd, tfar):
    """PhotonBeam::intersection (vol_primitives.rs:140-181): None or (u, v, w, sin_theta)."""
    with np.errstate(all="ignore"):
        d1d2c = _cross(rd, bd)
        sin_theta_sqr = _dot(d1d2c, d1d2c)
        ad = _dot(bo - ro, d1d2c)
        if F32(ad * ad) >= F32(F32(radius * radius) * sin_theta_sqr):
            return None
        d1d2 = _dot(rd, bd)
        d1d2_sqr = F32(d1d2 * d1d2)
        d1d2_sqr_minus1 = F32(d1d2_sqr - F32(1.0))
        if d1d2_sqr_minus1 < F32(1e-5) and d1d2_sqr_minus1 > F32(-1e-5):
            return None
        d1o1 = _dot(rd, ro)
        d1o2 = _dot(rd, bo)
        w = F32(F32(F32(d1o1 - d1o2) - F32(d1d2 * F32(_dot(bd, ro) - _dot(bd, bo)))) / d1d2_sqr_minus1)
        if w <= R.TNEAR or w >= tfar:
            return None
        v = F32(F32(F32(w + d1o1) - d1o2) / d1d2)
        if v <= F32(0.0) or v >= blen or not np.isfinite(v):
            return None
        sin_theta = F32(np.sqrt(sin_theta_sqr))
        u = F32(np.abs(ad) / sin_theta)
        return u, v, w, sin_theta


def _color_times(c, s):
    return (c * s).astype(np.float32) if np.isfinite(s) else np.zeros(3, np.float32)


def _contribute(rad, radius, medium, w, sin_theta):
    """PhotonBeam::contribute (vol_primitives.rs:184-199)."""
    sigma_t = (np.asarray(medium.sigma_a, np.float32) + np.asarray(medium.sigma_s, np.float32)) * F32(1.0)
    transmittance = B._expf(-_color_times(sigma_t, w))
    phase_func = np.asarray(medium.sigma_s, np.float32) * (F32(1.0) / (F32(np.pi) * F32(4.0)))
    weight = F32(F32(F32(1.0) / sin_theta) * F32(F32(0.5) / radius))
    return _color_times((rad * transmittance) * phase_func, weight)


def _scalar_gather(tree, sub, radius, medium, norm, ro, rd, tfar):
    """BHVAccel::gather (accel.rs:545-581) with its stack, then `c += contribute * norm_photon` in the order it returns the beams."""
    o, length, d, rad = R.records_of(sub)
    c = np.zeros(3, np.float32)
    accepted = 0
    stack = [] if tree["root"] is None else [tree["root"]]
    while stack:
        node = tree["nodes"][stack.pop()]
        if not B._box_entered(node["lo"], node["hi"], ro[None, :], rd[None, :], np.asarray([tfar], np.float32))[0]:
            continue
        if node["left"] is None and node["right"] is None:
            for place in range(node["first"], node["first"] + node["count"]):
                b = int(tree["order"][place])
                its = _intersection(o[b], d[b], length[b], F32(radius), ro, rd, tfar)
                if its is not None:
                    accepted += 1
                    c = c + _color_times(_contribute(rad[b], F32(radius), medium, its[2], its[3]), norm)
        else:
            if node["left"] is not None:
                stack.append(node["left"])
            if node["right"] is not None:
                stack.append(node["right"])
    return c, accepted


@pytest.mark.parametrize("seed,sigma_a,sigma_s", [(1, (0.0,) * 3, (1.0,) * 3), (2, (0.1, 0.2, 0.3), (0.9, 0.4, 0.0))])
def test_restatement_equals_the_scalar_walk(built, seed, sigma_a, sigma_s):
    rs = np.random.RandomState(seed)
    words = _random_beams(rs, 12, zero_every=5)
    medium = _medium(sigma_a, sigma_s)
    radius, n_paths = 0.4, 7
    ro, rd, tfar = _random_rays(rs, 160)
    sub = R.split(words)
    tree = R.build_tree(sub, radius)
    beams = R.Beams(sub, n_paths, radius, medium)
    c, _, accepted, _ = R.gather(tree, beams, ro, rd, tfar)
    total = 0
    for k in range(ro.shape[0]):
        want, n = _scalar_gather(tree, sub, radius, medium, beams.norm, ro[k], rd[k], tfar[k])
        np.testing.assert_array_equal(c[k].view(np.uint32), want.view(np.uint32), err_msg=f"ray {k}")
        total += n
    assert total == accepted and accepted >= 20


def test_tree_walk_against_all_beams(built):
    """The tree only prunes: every (ray, beam) pair it accepts is one the loop over all beams accepts, and the sums agree."""
    rs = np.random.RandomState(5)
    sub = R.split(_random_beams(rs, 40))
    ro, rd, tfar = _random_rays(rs, 256)
    beams = R.Beams(sub, 3, 0.2, _medium((0.0,) * 3, (1.0,) * 3))
    _, _, accepted, pairs = R.gather(R.build_tree(sub, 0.2), beams, ro, rd, tfar, want_pairs=True)
    tree_pairs = {(int(r), b) for rays, b, _ in pairs for r in rays}
    all_pairs = set()
    for b in range(sub.shape[0]):
        ok = beams.test(b, ro, rd, tfar)[0]
        all_pairs |= {(int(r), b) for r in np.nonzero(ok)[0]}
    assert accepted == len(tree_pairs) > 50 and tree_pairs == all_pairs


def test_closed_forms(built):
    """The ray from the origin along +z and a unit beam of direction (0, 0.6, 0.8) whose middle is (u, 0, 2): the lines pass at distance u, at w = 2 along the
    ray and v = 0.5 along the beam, under sin_theta = 0.6.  The reference's v = (w + d1o1 - d1o2) / d1d2 is 0 / 0 for a beam exactly perpendicular to the ray,
    which `!v.is_finite()` then drops: kept."""
    radius, u0 = 0.25, 0.125
    ro, rd = np.zeros((1, 3), np.float32), np.asarray([[0.0, 0.0, 1.0]], np.float32)
    tfar = np.asarray([10.0], np.float32)
    medium = _medium((0.0,) * 3, (0.5,) * 3)
    tilt = (0.0, 0.6, 0.8)

    def one(o, d, length, tf=tfar):
        beams = R.Beams(R.beam_words([o], length, [d], [(1.0, 2.0, 4.0)]), 1, radius, medium)
        return beams, beams.test(0, ro, rd, tf)

    def start(x, z, v=0.5):
        return (x, -0.6 * v, z - 0.8 * v)

    beams, (ok, u, v, w, sin_theta) = one(start(u0, 2.0), tilt, 1.0)
    assert ok[0]
    np.testing.assert_allclose([u[0], v[0], w[0], sin_theta[0]], [u0, 0.5, 2.0, 0.6], rtol=2e-6)
    c = beams.contribute(0, w, sin_theta)[0]
    want = np.asarray([1.0, 2.0, 4.0]) * math.exp(-0.5 * 2.0) * (0.5 / (4 * math.pi)) * (1 / 0.6) * (0.5 / radius)
    np.testing.assert_allclose(c, want, rtol=4e-6)
    # perpendicular at distance u: sin_theta = 1 and the kernel weight is 0.5 / r, but v is not finite and the beam is dropped
    _, (ok, u, _, w, sin_theta) = one((u0, -0.5, 2.0), (0.0, 1.0, 0.0), 1.0)
    assert not ok[0] and (u[0], w[0], sin_theta[0]) == (u0, 2.0, 1.0)
    assert not one(start(radius, 2.0), tilt, 1.0)[1][0][0]                           # at distance r exactly: `ad * ad >= r^2 sin^2` rejects
    assert not one((u0, 0.0, 1.0), (0.0, 0.0, 1.0), 1.0)[1][0][0]                    # parallel to the ray
    assert not one(start(u0, -2.0), tilt, 1.0)[1][0][0]                              # behind the ray's origin: w <= tnear
    assert not one(start(u0, 2.0), tilt, 1.0, np.asarray([1.9], np.float32))[1][0][0]      # past tfar: w >= tfar
    assert not one(start(u0, 2.0, -0.1), tilt, 1.0)[1][0][0]                         # the beam starts past the ray: v <= 0
    assert not one(start(u0, 2.0), tilt, 0.4)[1][0][0]                               # the beam ends before the ray: v >= length


# ---- the host's split and tree against the restatement, byte for byte
def _same_split_and_tree(words, radius, what):
    sub = api.beam_split(words)
    want = R.split(words)
    assert sub.shape == want.shape, (what, sub.shape, want.shape)
    np.testing.assert_array_equal(sub, want, err_msg=what)
    _same_tree(sub, radius, what)
    return sub


def _same_tree(sub, radius, what):
    got = api.beam_tree_build(sub, radius)
    assert_trees_equal(got, R.tree_arrays(R.build_tree(sub, radius)), what)
    return got


@pytest.mark.parametrize("n,seed", [(1, 0), (2, 1), (3, 2), (17, 3), (200, 4)])
def test_split_and_tree_of_random_beams(built, n, seed):
    rs = np.random.RandomState(seed)
    sub = _same_split_and_tree(_random_beams(rs, n, zero_every=7 if n > 7 else 0), 0.05, f"n = {n}")
    assert 5 * (n - (n + 6) // 7 if n > 7 else n) <= sub.shape[0] <= 6 * n
    lengths = R.records_of(sub)[1]
    assert (lengths > 0).all()                                                       # a beam of length 0 yields no sub-beam


@pytest.mark.parametrize("n_sub", [1, 2, 4, 5, 6, 9])
def test_tree_of_few_sub_beams(built, n_sub):
    """One leaf (1), a full leaf (4), the first inner node (5), odd splits."""
    rs = np.random.RandomState(10 + n_sub)
    boxes, links, _ = _same_tree(_random_beams(rs, n_sub), 0.02, f"n_sub = {n_sub}")
    assert (boxes.shape[0] == 1) == (n_sub <= 4)
    if n_sub <= 4:
        assert tuple(links[0]) == (1, 0, n_sub)


def test_one_beam_makes_five_sub_beams(built):
    words = R.beam_words([(0.0, 0.0, 0.0)], 1.0, [(0.0, 0.0, 1.0)], [(1.0, 1.0, 1.0)])
    sub = _same_split_and_tree(words, 0.01, "one beam")
    o, length, _, _ = R.records_of(sub)
    assert sub.shape[0] == 5 and (length == F32(1.0) / F32(5.0)).all()
    np.testing.assert_array_equal(o[:, 2], (np.arange(5, dtype=np.float32) * F32(1.0)) * (F32(1.0) / F32(5.0)))


def test_tree_keeps_the_order_of_equal_keys(built):
    """Duplicated sub-beams, and -0 beside +0 in a key: the stable-tie contract."""
    rs = np.random.RandomState(8)
    base = _random_beams(rs, 6)
    axis = R.beam_words([(0.0, 0.5, 0.5), (-0.0, 0.5, 0.5), (0.0, 0.5, 0.5)], 0.0, [(1.0, 0.0, 0.0)], [(1.0, 1.0, 1.0)])
    sub = np.concatenate([base, base[::-1], base, axis])
    assert not R.sort_keys_distinct(sub)
    _same_tree(sub, 0.1, "ties")


def test_size_only_call_and_capacities(built):
    import ctypes as C
    from rustlight_amd import abi
    words = _random_beams(np.random.RandomState(3), 9)
    want = R.split(words)
    n = C.c_size_t()
    L = api.lib()
    assert L.rl_beam_split(abi.u32ptr(words), 9, 0, C.byref(n), None) == api.RL_OK and n.value == want.shape[0]
    short = np.zeros((want.shape[0], api.BEAM_WORDS), np.uint32)
    assert L.rl_beam_split(abi.u32ptr(words), 9, want.shape[0] - 1, C.byref(n), abi.u32ptr(short)) == RL_ERR_INVALID_ARGUMENT
    assert not short.any()
    n_nodes = C.c_size_t()
    assert L.rl_beam_tree_build(abi.u32ptr(want), want.shape[0], 0.1, 0, C.byref(n_nodes), None, None, None) == api.RL_OK
    boxes, links, order = R.tree_arrays(R.build_tree(want, 0.1))
    assert n_nodes.value == boxes.shape[0]
    b, l, o = np.zeros_like(boxes), np.zeros_like(links), np.zeros_like(order)
    assert L.rl_beam_tree_build(abi.u32ptr(want), want.shape[0], 0.1, n_nodes.value - 1, C.byref(n_nodes), abi.fptr(b), abi.u32ptr(l), abi.u32ptr(o)) == RL_ERR_INVALID_ARGUMENT
    assert L.rl_beam_split(None, 0, 0, C.byref(n), None) == api.RL_OK and n.value == 0                 # nothing to split


def test_refused_inputs(built):
    words = _random_beams(np.random.RandomState(0), 8)
    for word in (1, 3, 5):                                        # o, length, d
        for bad in (float("nan"), float("inf")):
            w = words.copy()
            w[4, word] = np.float32(bad).view(np.uint32)
            with pytest.raises(api.RustlightError) as e:
                api.beam_split(w)
            assert e.value.code == RL_ERR_INVALID_ARGUMENT, (word, bad)
            with pytest.raises(api.RustlightError) as e:
                api.beam_tree_build(w, 0.1)
            assert e.value.code == RL_ERR_INVALID_ARGUMENT, (word, bad)
    zero = words.copy()
    zero.view(np.float32)[:, 3] = 0.0                             # no beam has a length: avg_split = 0
    with pytest.raises(api.RustlightError) as e:
        api.beam_split(zero)
    assert e.value.code == RL_ERR_INVALID_ARGUMENT
    huge = words.copy()
    huge.view(np.float32)[:, 3] = 3.0e38                          # the sum of the lengths overflows: avg_split = inf
    with pytest.raises(api.RustlightError) as e:
        api.beam_split(huge)
    assert e.value.code == RL_ERR_INVALID_ARGUMENT
    far = words.copy()
    far.view(np.float32)[2, 0] = 3.0e38                           # finite words whose box is not: (o + d * length) + r overflows
    far.view(np.float32)[2, 4] = 3.0e38
    with pytest.raises(api.RustlightError) as e:
        api.beam_tree_build(far, 0.1)
    assert e.value.code == RL_ERR_INVALID_ARGUMENT
    for radius in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(api.RustlightError) as e:
            api.beam_tree_build(words, radius)
        assert e.value.code == RL_ERR_INVALID_ARGUMENT, radius


def test_classes(built):
    """The new class stands beside IntegratorVolPrimitives, which keeps refusing the primitive."""
    with pytest.raises(api.RustlightError):
        api.IntegratorVolPrimitives(primitives="beam")
    integ = api.IntegratorPhotonBeams(nb_primitive=64, max_depth=4, rr_depth=2, radius=0.05, light_streams="per_path")
    assert (integ.nb_primitive, integ.max_depth, integ.rr_depth, integ.radius, integ.light_streams) == (64, 4, 2, 0.05, "per_path")
    with pytest.raises(ValueError):
        api.IntegratorPhotonBeams(light_streams="other")
    assert api.BEAM_WORDS == 12 and api.BEAM_MAX == 1 << 17
