"""Shared by the photon-tree tests: the position families the device build is held to the host build on (random, heavily tied, all equal, and mixed
scales from denormals to 1e30), records made from positions, and a numpy
level-by-level build — the CPU-side model of kernels/phototree.hip.h.  The model uses only what the kernels use: the closed-form topology (a function of n
alone) and, per range, an UNSTABLE sort by the unique pair (ordered key of pos[axis], place before the sort)."""
import numpy as np

from rustlight_amd import api

RADIUS = 0.2
FAMILIES = ("normal", "tied", "point", "scales")


def positions(family, n, seed=0):
    rng = np.random.default_rng(seed * 1000003 + n)
    if family == "normal":
        return rng.standard_normal((n, 3)).astype(np.float32)
    if family == "tied":                       # few distinct values per axis, and -0.0 beside +0.0 on x: ties and the two zeros fall on the sort axis
        p = (np.round(rng.standard_normal((n, 3)) * 2.0) / 2.0).astype(np.float32)
        p[::3, 0] = np.float32(-0.0)
        return p
    if family == "point":                      # every sort is all ties, every extent equal
        return np.tile(np.array([[0.25, -1.5, 3.0]], np.float32), (n, 1))
    if family == "scales":                     # f32 denormals, values near +-1e30 and ordinary ones mixed per coordinate, all finite: a denormal p gives p - r == -r and
        kind = rng.integers(0, 3, (n, 3))      # p + r == r exactly, so boxes tie where the sort keys do not, and beside 1e30 every other extent vanishes
        sign = np.where(rng.integers(0, 2, (n, 3)) == 1, np.uint32(0x80000000), np.uint32(0))
        tiny = (rng.integers(1, 1 << 23, (n, 3)).astype(np.uint32) | sign).view(np.float32)
        huge = (np.float32(1.0e30) * (1.0 + 0.01 * rng.standard_normal((n, 3))).astype(np.float32)) * np.where(sign != 0, np.float32(-1.0), np.float32(1.0))
        p = np.where(kind == 0, tiny, np.where(kind == 1, huge.astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32))).astype(np.float32)
        assert np.isfinite(p).all()
        return p
    raise ValueError(family)


def words_of(pos, kind=1):
    """Volume records ([n, VPL_WORDS] u32) at `pos`, with radiance and direction filled so that a wrong gather shows."""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    n = pos.shape[0]
    w = np.zeros((n, api.VPL_WORDS), np.uint32)
    w[:, 0] = kind
    w[:, 4:7] = pos.view(np.uint32)
    w[:, 7:10] = (np.arange(3 * n, dtype=np.float32).reshape(n, 3) + 1.0).view(np.uint32)
    w[:, 10:13] = (np.arange(3 * n, dtype=np.float32).reshape(n, 3) * -0.5).view(np.uint32)
    return w


def node_count(m):
    """N(m), the closed form of pt_node_count: a level holds ranges of two sizes only, s (c0 of them) and s + 1 (c1 of them)."""
    if m <= 4:
        return 1 if m else 0
    s, c0, c1, total = m, 1, 0, 0
    while True:
        total += c0 + c1
        if s + 1 <= 4 or (s <= 4 and c1 == 0):
            return total
        if s == 4:
            return total + 2 * c1
        if s & 1:
            c1, s = c0 + 2 * c1, (s - 1) // 2
        else:
            c0, s = 2 * c0 + c1, s // 2


def node_count_recursive(m):
    return 1 if m <= 4 else 1 + node_count_recursive(m - m // 2) + node_count_recursive(m // 2)


def sort_key(x):
    """The ordered key of an f32 array: -0 -> +0, then negative -> all bits inverted, else the sign bit set."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    return np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def levels_build(pos, radius, rng=None):
    """(boxes, links, order) level by level.  Every level is a list of disjoint ranges (b, e, node index) known from n alone; rng, if given, shuffles the
    composite keys before they are sorted, so that nothing can lean on the sort being stable or on the order of arrival."""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    n = pos.shape[0]
    r = np.float32(radius)
    n_nodes = node_count(n)
    boxes, links, order = np.zeros((n_nodes, 6), np.float32), np.zeros((n_nodes, 3), np.uint32), np.arange(n, dtype=np.uint32)
    level = [(0, n, 0)] if n else []
    while level:
        nxt = []
        new_order = order.copy()
        for b, e, node in level:
            m = e - b
            p = pos[order[b:e]]
            lo, hi = np.minimum(p - r, p + r).min(axis=0), np.maximum(p - r, p + r).max(axis=0)
            boxes[node] = np.concatenate([lo, hi])
            if m <= 4:
                links[node] = (node + 1, b, m)
                continue
            links[node] = (node + node_count(m), 0, 0)
            sx, sy, sz = hi - lo
            axis = (0 if sx > sz else 2) if sx > sy else (1 if sy > sz else 2)
            comp = (sort_key(p[:, axis]).astype(np.uint64) << np.uint64(32)) | np.arange(b, e, dtype=np.uint64)      # (key, place): unique
            if rng is not None:
                comp = rng.permutation(comp)
            comp = np.sort(comp)                                                                                      # any sort
            new_order[b:e] = order[(comp & np.uint64(0xffffffff)).astype(np.int64)]
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
