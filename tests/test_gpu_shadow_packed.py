"""The packed shadow stage of the persistent kernel's tail form (trace.hip.h: occluded_packed): the shadow rays of a wave enumerate their candidate leaves first,
then the (ray, leaf) pairs are dealt to the lanes densely.  It is another schedule of the same any-hit queries: every verdict, hence every image byte and counter,
is that of the per-lane loop.  Segment level through the hook Context.visible_lds (both forms on a scene staged in LDS), render level through the options that force
the tail form (fused_tail_blocks / fused_tail_split) against fused_tail_blocks = 0; option shadow_pack_capacity makes small scenes reach the flush."""
import dataclasses

import numpy as np
import pytest

from rustlight_amd import api, scenes
from tests.test_fused_tail_split import COUNTERS

pytestmark = pytest.mark.gpu

N_FENCE = 41


def _tri_scene(n_tris):
    """A scene whose BVH root is a leaf: one emissive mesh of n_tris (1 or 2) triangles."""
    v = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.25]], np.float32)
    idx = np.asarray([[0, 1, 2], [1, 3, 2]][:n_tris], np.uint32)
    m = scenes.MeshData("leaf", v, idx, None, None, scenes.matte((0.5, 0.5, 0.5)), emission=(1.0, 1.0, 1.0))
    to_world = np.asarray([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0.25, 0.25, -3, 1], dtype=np.float32)
    return scenes.SceneData(32, 32, 40.0, 0, to_world, False, [m])


def fence_scene(width=64, height=64):
    """N_FENCE thin slabs in the planes x = const, each a narrow diagonal band across the rectangle y in [0, 1], z in [-0.5, 0.5]: a segment along x passes the
    bounding box of every slab (41 candidate leaves, more than a lane's list holds) and meets few of the bands.  A floor under them and a light at x = 1.3 that
    shines along -x through the slabs; the Cornell box's camera."""
    white = scenes.matte((0.7, 0.7, 0.7))
    meshes = [scenes._quad_mesh("Floor", [-1.5, 0, -2, -1.5, 0, 2, 1.5, 0, 2, 1.5, 0, -2], [0, 1, 0], white),
              scenes._quad_mesh("Light", [1.3, 0.2, -0.4, 1.3, 0.2, 0.4, 1.3, 0.8, 0.4, 1.3, 0.8, -0.4], [-1, 0, 0], scenes.matte((0, 0, 0)), emission=(40.0, 40.0, 40.0))]
    for i in range(N_FENCE):
        x = -1.0 + 0.05 * i
        w = 0.03
        meshes.append(scenes._quad_mesh(f"Slab{i}", [x, 0, -0.5, x, w, -0.5, x, 1, 0.5, x, 1 - w, 0.5], [1, 0, 0], white))
    return scenes.SceneData(width, height, scenes.CBOX_FOV, 1, np.asarray(scenes.CBOX_TO_WORLD, dtype=np.float32), False, meshes)


def _triangles(sd):
    return np.concatenate([m.vertices[m.indices.astype(np.int64)] for m in sd.meshes]).astype(np.float32)        # (n, 3, 3)


def segments(sd, seed):
    """About 64 k segments: random ones, ones parallel to an axis that start on a plane of the scene's box, ones that graze the box's faces, ones that end or start on
    a triangle, and ones of zero length."""
    rng = np.random.default_rng(seed)
    tris = _triangles(sd)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    ext = np.maximum(hi - lo, 0.5)

    def inside(n, grow=0.1):
        return (lo - grow * ext + rng.random((n, 3)) * (1 + 2 * grow) * ext).astype(np.float32)

    parts = [(inside(24576), inside(24576))]
    # parallel to an axis, the origin on a plane of the box (exactly: the plane's own f32)
    n = 12288
    p0 = inside(n, 0.0)
    plane_axis, side, run_axis = rng.integers(0, 3, n), rng.integers(0, 2, n), rng.integers(0, 3, n)
    p0[np.arange(n), plane_axis] = np.where(side == 1, hi[plane_axis], lo[plane_axis])
    p1 = p0.copy()
    p1[np.arange(n), run_axis] += (rng.choice([-1.0, 1.0], n) * rng.random(n) * 2.5 * ext[run_axis]).astype(np.float32)
    parts.append((p0, p1))
    # grazing: both ends within a few ulps .. 1e-4 of the same face of the box
    n = 8192
    a, b = inside(n, 0.0), inside(n, 0.0)
    ax, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
    face = np.where(side == 1, hi[ax], lo[ax])
    off = (rng.choice([-1.0, 1.0], (2, n)) * 10.0 ** rng.uniform(-7, -4, (2, n))).astype(np.float32)
    a[np.arange(n), ax] = face + off[0]
    b[np.arange(n), ax] = face + off[1]
    parts.append((a, b))
    # one end on a triangle (a point of its plane inside it, or on an edge / a corner)
    n = 16384
    t = tris[rng.integers(0, len(tris), n)]
    u, v = rng.random(n), rng.random(n)
    fold = u + v > 1
    u, v = np.where(fold, 1 - u, u), np.where(fold, 1 - v, v)
    edge = rng.random(n) < 0.15
    v = np.where(edge, 0.0, v)
    u = np.where(rng.random(n) < 0.05, 0.0, u)
    on = (t[:, 0] + u[:, None] * (t[:, 1] - t[:, 0]) + v[:, None] * (t[:, 2] - t[:, 0])).astype(np.float32)
    other = inside(n)
    swap = rng.random(n) < 0.5
    parts.append((np.where(swap[:, None], on, other), np.where(swap[:, None], other, on)))
    # zero length
    z = inside(2048)
    z[:1024] = on[:1024]
    parts.append((z, z.copy()))
    p0 = np.ascontiguousarray(np.concatenate([p[0] for p in parts]), np.float32)
    p1 = np.ascontiguousarray(np.concatenate([p[1] for p in parts]), np.float32)
    return p0, p1


SEGMENT_SCENES = {
    "cbox": lambda: scenes.cbox(64, 64),
    "leaf1": lambda: _tri_scene(1),
    "leaf2": lambda: _tri_scene(2),
    "fence": fence_scene,
    "many_lights42": lambda: scenes.many_lights(64, 48, n=2, use_ats=False),
    "many_lights52": lambda: scenes.many_lights(64, 48, n=3, use_ats=False),
}


@pytest.mark.parametrize("name", list(SEGMENT_SCENES))
def test_packed_verdicts_equal_the_per_lane_loop(built, name):
    """Every segment, both forms, the default capacity and capacities 1 and 2 (a flush after every leaf or two); the per-lane loop on the staged scene also agrees
    with rl_visible_batch, which streams the same BVH."""
    sd = SEGMENT_SCENES[name]()
    ctx = api.Context(api.Scene(sd), 0)
    assert ctx.debug_sizes()["lds_scene"]
    p0, p1 = segments(sd, seed=len(name))
    assert len(p0) > 60000
    ref = ctx.visible_lds(p0, p1, packed=False)
    np.testing.assert_array_equal(ref, ctx.visible(p0, p1))
    if name in ("cbox", "fence"):
        assert 0.05 < ref.mean() < 0.95                                   # both verdicts are common
    for cap in (0, 1, 2):
        got = ctx.visible_lds(p0, p1, packed=True, capacity=cap)
        bad = np.flatnonzero(got != ref)
        assert bad.size == 0, (name, cap, bad.size, bad[:8], p0[bad[:2]], p1[bad[:2]])
    # a batch that is no multiple of the wave: the last wave's idle lanes hold no segment
    np.testing.assert_array_equal(ctx.visible_lds(p0[:1000 + 37], p1[:1000 + 37], packed=True), ref[:1037])


def test_fence_segments_overflow_a_lanes_list(built):
    """Segments along x through all the slabs: 41 candidate leaves per segment, more than any stack has levels — the wave flushes with the default capacity too.
    Those that pass between the bands are visible, those through a band are not."""
    sd = fence_scene()
    ctx = api.Context(api.Scene(sd), 0)
    assert ctx.debug_sizes()["lds_scene"] and ctx.debug_sizes()["stack_depth"] < N_FENCE
    rng = np.random.default_rng(5)
    n = 4096
    y, z = rng.uniform(0.02, 0.98, n).astype(np.float32), rng.uniform(-0.48, 0.48, n).astype(np.float32)
    p0 = np.stack([np.full(n, -1.2, np.float32), y, z], 1)
    p1 = np.stack([np.full(n, 1.2, np.float32), y, z], 1)
    ref = ctx.visible_lds(p0, p1, packed=False)
    assert 0.1 < ref.mean() < 0.99
    for cap in (0, 1, 2, 5):
        np.testing.assert_array_equal(ctx.visible_lds(p0, p1, packed=True, capacity=cap), ref)
    # mixed into a batch of short segments that cross nothing: waves where one lane fills its list and the others hold none
    q0, q1 = np.tile(np.asarray([[0.0, 1.5, 0.0]], np.float32), (n, 1)), np.tile(np.asarray([[0.1, 1.6, 0.0]], np.float32), (n, 1))
    pick = rng.random(n) < 0.03
    m0, m1 = np.where(pick[:, None], p0, q0), np.where(pick[:, None], p1, q1)
    np.testing.assert_array_equal(ctx.visible_lds(m0, m1, packed=True), ctx.visible_lds(m0, m1, packed=False))


class Pair:
    """One context: the frame without a tail (the per-lane loop, kept) against the tail form (the packed stage)."""

    def __init__(self, sd, seed=3):
        self.ctx = api.Context(api.Scene(sd), 0)
        self.seeds = api.IndependentSampler(seed).block_seeds(sd.width, sd.height)

    def check(self, T=1000, S=2, cap=None, expect_tail=True, **kw):
        with self.ctx.options(fused_tail_blocks=0):
            ref, rst = self.ctx.render(self.seeds, api.path_params(**kw))
        with self.ctx.options(fused_tail_blocks=T, fused_tail_split=S, shadow_pack_capacity=cap):
            img, st = self.ctx.render(self.seeds, api.path_params(**kw))
        assert img.tobytes() == ref.tobytes(), (T, S, cap, kw)
        for k in COUNTERS:
            assert st[k] == rst[k], (k, st[k], rst[k], T, S, cap, kw)
        if expect_tail:           # the tail form did run: one lane per pixel + the tail's fold
            with self.ctx.options(fused_tail_blocks=0):
                one_lane = self.ctx.render(self.seeds, api.path_params(sample_split=1, **kw))[1]["kernel_launches"]
            assert st["kernel_launches"] == one_lane + 1, (st["kernel_launches"], one_lane)
        return img, st, rst


@pytest.mark.parametrize("cap", [None, 1, 2])
@pytest.mark.parametrize("numerics", [0, 1])
def test_render_cbox(built, cap, numerics):
    """96 x 64: the box in the middle columns, background blocks at the sides (waves that hold no shadow ray at all beside waves that do); exact and tolerance build."""
    p = Pair(scenes.cbox(96, 64))
    img, st, rst = p.check(T=1000, S=2, cap=cap, spp=6, numerics=numerics)
    assert img.mean() > 0.05 and st["shadow_rays"] > 0
    p.check(T=3, S=4, cap=cap, spp=5, numerics=numerics)


@pytest.mark.parametrize("cap", [None, 1])
def test_render_fence(built, cap):
    """The floor lit through the slabs: shadow rays with dozens of candidate leaves."""
    p = Pair(fence_scene(96, 64))
    img, st, _ = p.check(T=1000, S=2, cap=cap, spp=8)
    assert img.mean() > 0.01 and st["shadow_rays"] > 0


def test_render_without_shadow_rays(built):
    """The camera turned away from the box: no wave ever holds a shadow ray."""
    sd = scenes.cbox(64, 64)
    away = np.array(sd.to_world, dtype=np.float32).copy()
    away[0:3], away[8:11] = (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
    img, st, _ = Pair(dataclasses.replace(sd, to_world=away)).check(T=7, S=4, expect_tail=False, spp=4)
    assert not img.any() and st["shadow_rays"] == 0


def test_render_capacity_one_equals_the_default(built):
    p = Pair(scenes.cbox(128, 128), seed=8)
    with p.ctx.options(fused_tail_blocks=1000, fused_tail_split=4):
        a, sa = p.ctx.render(p.seeds, api.path_params(spp=4))
        with p.ctx.options(shadow_pack_capacity=1):
            b, sb = p.ctx.render(p.seeds, api.path_params(spp=4))
    assert a.tobytes() == b.tobytes() and all(sa[k] == sb[k] for k in COUNTERS)
