"""Shared by the plane-tree tests: the plane families the device build (kernels/planetree.hip) is held to the host build (host/planetree.cpp) on, as records
of PLANE_WORDS u32, and numpy forms of a plane's corners and middle in the host's arithmetic (every operation a separately rounded f32), with which
tests/test_plane_device_resources.py checks on the CPU that the families hold what they are for: box coordinates that are -0 and +0, and tied sort keys;
and levels_build, a numpy level-by-level build that is the CPU-side model of the plane kernels (their minimum on (value, last place) and their unstable sort)."""
import numpy as np

from rustlight_amd import api

FAMILIES = ("random", "equal", "tied", "degenerate", "zeros")
NEG_ZERO = np.uint32(0x80000000)


def records(o, d0, d1, l0, l1):
    """[n, PLANE_WORDS] u32 from o, d0, d1 ([n, 3]) and length0, length1 ([n]); weight, sample, type and id_emitter filled so that a wrong order shows."""
    o, d0, d1 = (np.ascontiguousarray(v, np.float32).reshape(-1, 3) for v in (o, d0, d1))
    n = o.shape[0]
    w = np.zeros((n, api.PLANE_WORDS), np.uint32)
    w[:, 0:3], w[:, 3:6], w[:, 6:9] = o.view(np.uint32), d0.view(np.uint32), d1.view(np.uint32)
    w[:, 9], w[:, 10] = np.asarray(l0, np.float32).view(np.uint32), np.asarray(l1, np.float32).view(np.uint32)
    w[:, 11:14] = (np.arange(3 * n, dtype=np.float32).reshape(n, 3) + 1.0).view(np.uint32)
    w[:, 14:16] = (np.arange(2 * n, dtype=np.float32).reshape(n, 2) * 0.25).view(np.uint32)
    w[:, 16] = np.arange(n, dtype=np.uint32) % 4
    w[:, 17] = np.arange(n, dtype=np.uint32) % 3
    return w


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def planes(family, n, seed=0):
    rng = np.random.default_rng(seed * 1000003 + n + 17)
    if family == "random":
        return records(rng.standard_normal((n, 3)), _unit(rng.standard_normal((n, 3))), _unit(rng.standard_normal((n, 3))),
                       rng.uniform(0.1, 2.0, n), rng.uniform(0.1, 2.0, n))
    if family == "equal":                      # every sort is all ties, every extent equal
        one = np.array([[0.25, -1.5, 3.0]], np.float32)
        return records(np.tile(one, (n, 1)), np.tile([[1.0, 0.0, 0.0]], (n, 1)), np.tile([[0.0, 0.6, 0.8]], (n, 1)), np.full(n, 0.5), np.full(n, 1.5))
    if family == "tied":                       # axis-aligned planes on a coarse grid: few distinct middles per axis, and many planes with the same box
        o = np.round(rng.standard_normal((n, 3)) * 2.0) / 2.0
        eye = np.eye(3, dtype=np.float32)
        a = rng.integers(0, 3, n)
        return records(o, eye[a], eye[(a + 1 + rng.integers(0, 2, n)) % 3], rng.integers(1, 3, n) * 0.5, rng.integers(1, 3, n) * 0.5)
    if family == "degenerate":                 # a third with length0 = 0 (a segment), a third with d0 = d1 (a segment of two lengths), the rest ordinary
        d0, d1 = _unit(rng.standard_normal((n, 3))), _unit(rng.standard_normal((n, 3)))
        l0 = rng.uniform(0.1, 2.0, n)
        kind = np.arange(n) % 3
        l0[kind == 0] = 0.0
        d1[kind == 1] = d0[kind == 1]
        return records(np.round(rng.standard_normal((n, 3))), d0, d1, l0, rng.uniform(0.1, 2.0, n))
    if family == "zeros":
        # Corners that are -0 beside +0 on every axis.  o is -0 or +0, the directions hold -0, +0 and one sign of 1 per axis (x: +1, y: -1, z: both), the lengths
        # 0, 0.5 and 1: so on x every corner is >= 0 and a box's minimum there is a zero, on y every corner is <= 0 and the maximum is a zero, and which zero
        # it is depends on the order the corners and the planes are taken in.  Planes whose extent vanishes on an axis make both ends of the box zeros.
        pick = lambda vals, shape: np.asarray(vals, np.float32)[rng.integers(0, len(vals), shape)]
        o = pick([-0.0, 0.0], (n, 3))
        d0, d1 = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        for d in (d0, d1):
            d[:, 0] = pick([-0.0, 0.0, 1.0], n)
            d[:, 1] = pick([-0.0, 0.0, -1.0], n)
            d[:, 2] = pick([-0.0, 0.0, 1.0, -1.0], n)
        return records(o, d0, d1, pick([0.0, 0.5, 1.0], n), pick([0.0, 0.5, 1.0], n))
    raise ValueError(family)


def _f(words, k):
    return np.ascontiguousarray(words[:, k]).view(np.float32)


def corners(words):
    """[n, 3, 4] f32: per axis o, o + d0 l0, o + d1 l1, (o + d0 l0) + d1 l1, as host/planetree.cpp's PlaneElems::corners takes them."""
    out = np.zeros((words.shape[0], 3, 4), np.float32)
    for a in range(3):
        o, e0, e1 = _f(words, a), _f(words, 3 + a) * _f(words, 9), _f(words, 6 + a) * _f(words, 10)
        out[:, a, 0], out[:, a, 1], out[:, a, 2] = o, o + e0, o + e1
        out[:, a, 3] = out[:, a, 1] + e1
    return out


def middles(words):
    """[n, 3] f32: (o + (d0 l0) 0.5) + (d1 l1) 0.5."""
    half = np.float32(0.5)
    return np.stack([(_f(words, a) + (_f(words, 3 + a) * _f(words, 9)) * half) + (_f(words, 6 + a) * _f(words, 10)) * half for a in range(3)], axis=1)


def _host_chain(values, take_min):
    """std::fmin / std::fmax over `values` in order from -+FLT_MAX, as the host build's libm takes them: of two equal values (zeros of different sign) the second."""
    acc = np.float32(3.402823466e+38 if take_min else -3.402823466e+38)
    for v in values:
        acc = (acc if acc < v else v) if take_min else (acc if acc > v else v)
    return np.float32(acc)


def levels_build(words, rng=None):
    """(boxes, links, order) level by level: the CPU-side model of the plane instantiation of kernels/phototree.hip.h.  It uses only what the kernels use: the
    closed-form topology, per plane the 6 box floats and 3 keys of the prepass, per range a minimum over (value with -0 -> +0, then the LAST place, which
    brings its zero's sign) and an UNSTABLE sort by the unique pair (ordered key of the middle, place); rng shuffles both before they are reduced."""
    from tests.photon_tree_cases import node_count, sort_key
    n = words.shape[0]
    c, mid = corners(words), middles(words)
    e_lo = np.array([[_host_chain(c[i, a], True) for a in range(3)] for i in range(n)], np.float32).reshape(n, 3)
    e_hi = np.array([[_host_chain(c[i, a], False) for a in range(3)] for i in range(n)], np.float32).reshape(n, 3)

    def reduce(vals, take_min):                                                # vals in place order
        places = np.arange(len(vals))
        if rng is not None:
            places = rng.permutation(places)
        best = None
        for pl in places:
            v = vals[pl]
            key = (float(v) + 0.0 if take_min else -(float(v) + 0.0), -pl)      # -0 + 0 = +0: the two zeros tie on the value; then the last place
            if best is None or key < best[0]:
                best = (key, v)
        return best[1]

    n_nodes = node_count(n)
    boxes, links, order = np.zeros((n_nodes, 6), np.float32), np.zeros((n_nodes, 3), np.uint32), np.arange(n, dtype=np.uint32)
    level = [(0, n, 0)] if n else []
    while level:
        nxt, new_order = [], order.copy()
        for b, e, node in level:
            m, el = e - b, order[b:e]
            lo = np.array([reduce(e_lo[el, a], True) for a in range(3)], np.float32)
            hi = np.array([reduce(e_hi[el, a], False) for a in range(3)], np.float32)
            boxes[node] = np.concatenate([lo, hi])
            if m <= 4:
                links[node] = (node + 1, b, m)
                continue
            links[node] = (node + node_count(m), 0, 0)
            sx, sy, sz = hi - lo
            axis = (0 if sx > sz else 2) if sx > sy else (1 if sy > sz else 2)
            comp = (sort_key(mid[el, axis]).astype(np.uint64) << np.uint64(32)) | np.arange(b, e, dtype=np.uint64)
            if rng is not None:
                comp = rng.permutation(comp)
            new_order[b:e] = order[(np.sort(comp) & np.uint64(0xffffffff)).astype(np.int64)]
            split = (b + e) // 2
            nxt.append((split, e, node + 1))
            nxt.append((b, split, node + 1 + node_count(m - m // 2)))
        order, level = new_order, nxt
    return boxes, links, order


def assert_trees_equal(got, want, what=""):
    for name, g, w in zip(("boxes", "links", "order"), got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)        # the bits: -0 and +0 differ
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")
