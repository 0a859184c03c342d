"""The tail of the persistent kernel's static tile order (options fused_tail_blocks = T, fused_tail_split = S; PathRender::plan_tail): the last T blocks that can see
the scene run at S lanes per pixel, their samples parked and folded in sample order.  It is another launch shape of the same render: image bytes and every counter
are those of the render without it; what it adds is one launch (the fold over the tail's pixels).  The forms that get no tail ignore the options."""
import dataclasses
import json
import os
import zlib

import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes

pytestmark = pytest.mark.gpu

COUNTERS = ("camera_samples", "vertices", "extension_rays", "shadow_rays", "rng_draws", "iterations", "n_extend_launches", "chunks", "overlapped")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Frame:
    """One context of a scene, the renders without a tail kept per parameter set (computed once, never changed)."""

    def __init__(self, sd, seed=3):
        self.sd = sd
        self.ctx = api.Context(api.Scene(sd), 0)
        self.seeds = api.IndependentSampler(seed).block_seeds(sd.width, sd.height)
        self._plain = {}

    def plain(self, **kw):
        key = tuple(sorted(kw.items()))
        if key not in self._plain:
            with self.ctx.options(fused_tail_blocks=0):
                img, st = self.ctx.render(self.seeds, api.path_params(**kw))
            img.setflags(write=False)
            self._plain[key] = (img, st)
        return self._plain[key]

    def tail(self, T, S, **kw):
        with self.ctx.options(fused_tail_blocks=T, fused_tail_split=S):
            return self.ctx.render(self.seeds, api.path_params(**kw))

    def one_lane_launches(self, **kw):
        """kernel_launches of the frame at one lane per pixel, no tail (a small frame's automatic choice is several lanes for every pixel + the fold)"""
        with self.ctx.options(fused_tail_blocks=0):
            return self.ctx.render(self.seeds, api.path_params(sample_split=1, **kw))[1]["kernel_launches"]

    def check(self, T, S, expect_tail, **kw):
        """expect_tail True: one lane per pixel + the tail + its fold; False: one lane per pixel, nothing parked, no fold; None: the options do not apply — the plan without them"""
        ref, rst = self.plain(**kw)
        img, st = self.tail(T, S, **kw)
        assert img.tobytes() == ref.tobytes(), (T, S, kw)
        for k in COUNTERS:
            assert st[k] == rst[k], (k, st[k], rst[k], T, S, kw)
        want = rst["kernel_launches"] if expect_tail is None else self.one_lane_launches(**kw) + (1 if expect_tail else 0)
        assert st["kernel_launches"] == want, (st["kernel_launches"], want, T, S, kw)
        return img, st


@pytest.fixture(scope="module")
def cbox96(built):
    return Frame(scenes.cbox(96, 64))          # 6 x 4 blocks, the box in the middle columns


@pytest.fixture(scope="module")
def cbox_ragged(built):
    return Frame(scenes.cbox(70, 50))          # the last block row and column are partial: 6 x 16, 16 x 2 and 6 x 2 pixels


@pytest.mark.parametrize("spp", [8, 5, 1])
@pytest.mark.parametrize("T", [1, 7, 1000])
@pytest.mark.parametrize("S", [2, 4, 8])
def test_tail_renders_the_same_frame(cbox96, S, T, spp):
    """S lanes per pixel on the last T heavy blocks (1000: all of them, and more than there are), spp a multiple of S, not a multiple of S, and below S (the lanes
    per pixel are then the largest power of two <= spp; at spp = 1 that is one lane: no tail)."""
    img, _ = cbox96.check(T, S, expect_tail=True if spp >= 2 else None, spp=spp)
    assert img.mean() > 0.05


@pytest.mark.parametrize("spp", [8, 5, 1])
@pytest.mark.parametrize("T", [1, 7, 1000])
@pytest.mark.parametrize("S", [2, 4, 8])
def test_tail_on_a_ragged_frame(cbox_ragged, S, T, spp):
    cbox_ragged.check(T, S, expect_tail=True if spp >= 2 else None, spp=spp)


@pytest.mark.parametrize("S", [2, 8])
def test_tail_follows_the_shards_own_blocks(cbox96, S):
    """Shard 1 of 2 owns every other block: the tail is the last heavy blocks of THAT list, the pixel items in between are the shard's."""
    for T in (1, 5, 1000):
        cbox96.check(T, S, expect_tail=True, spp=6, shard_index=1, shard_count=2)
    # ... and on the ragged frame, where the shard's last blocks are partial ones
    Frame(scenes.cbox(70, 50)).check(3, S, expect_tail=True, spp=5, shard_index=1, shard_count=2)


def test_frame_of_background_blocks_has_no_tail(built):
    """A camera that looks past the box: every block is background, so no block is marked, no sample is parked and no fold is launched (kernel_launches of the
    render without a tail) — and likewise a sensor that is never expanded (max_depth = 1)."""
    sd = scenes.cbox(96, 64)
    away = np.array(sd.to_world, dtype=np.float32).copy()
    away[0:3], away[8:11] = (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)        # the camera turned a quarter round: it looks along +x, past the box
    f = Frame(dataclasses.replace(sd, to_world=away))
    img, st = f.check(7, 4, expect_tail=False, spp=4)
    assert not img.any() and st["rng_draws"] == 2 * st["camera_samples"]
    Frame(sd).check(7, 4, expect_tail=False, spp=4, max_depth=1)
    assert f.one_lane_launches(spp=4) + 1 == f.plain(spp=4)[1]["kernel_launches"]          # (the plan without the options parks every pixel and folds)


def test_options_off_is_the_plan_without_a_tail(cbox96):
    """fused_tail_blocks = 0 (and fused_tail_split = 0 or 1): the same launches as a context that never heard of the options (at this size the automatic choice is
    no tail either)."""
    fresh = api.Context(api.Scene(cbox96.sd), 0)
    img0, st0 = fresh.render(cbox96.seeds, api.path_params(spp=8))
    ref, rst = cbox96.plain(spp=8)
    assert img0.tobytes() == ref.tobytes() and st0["kernel_launches"] == rst["kernel_launches"]
    for T, S in ((0, 4), (7, 0), (7, 1)):
        cbox96.check(T, S, expect_tail=None, spp=8)
    # a caller's own lanes per pixel (sample_split) keep their whole-frame form
    a, sta = cbox96.tail(7, 4, spp=8, sample_split=2)
    with cbox96.ctx.options(fused_tail_blocks=0):
        b, stb = cbox96.ctx.render(cbox96.seeds, api.path_params(spp=8, sample_split=2))
    assert a.tobytes() == ref.tobytes() and b.tobytes() == ref.tobytes() and sta["kernel_launches"] == stb["kernel_launches"]


def test_parking_buffer_only_where_a_tail_is(built):
    """A frame whose plan without the options is one lane per pixel (1920 x 1080: 8100 workgroups), a fresh context each: options off and a frame of background blocks
    allocate no parking buffer at all; the tail on allocates its own pixels x spp x 12 bytes — the run of the owned order from the first to the last of the T heavy
    blocks — and where that buffer cannot be had (test option fused_tail_no_buffer_test) the frame renders without a tail, without a buffer and without an error."""
    W, H, spp, T = 1920, 1080, 2, 512
    sd = scenes.cbox(W, H)
    seeds = api.IndependentSampler(4).block_seeds(W, H)
    off = api.Context(api.Scene(sd), 0)
    off.set_option("fused_tail_blocks", 0)
    ref, rst = off.render(seeds, api.path_params(spp=spp))
    assert off.sample_buf_bytes() == 0
    away = np.array(sd.to_world, dtype=np.float32).copy()
    away[0:3], away[8:11] = (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
    bg = api.Context(api.Scene(dataclasses.replace(sd, to_world=away)), 0)
    bg.set_option("fused_tail_blocks", T)
    img, st = bg.render(seeds, api.path_params(spp=spp))
    assert bg.sample_buf_bytes() == 0 and not img.any() and st["kernel_launches"] == rst["kernel_launches"]
    on = api.Context(api.Scene(sd), 0)
    on.set_option("fused_tail_blocks", T)
    img, st = on.render(seeds, api.path_params(spp=spp))
    assert img.tobytes() == ref.tobytes() and st["kernel_launches"] == rst["kernel_launches"] + 1
    # the T heavy blocks are whole ones or the partial ones of the last block row (16 x 8 pixels); blocks in between that see nothing come along: at most one in eight here
    assert T * 128 * spp * 12 <= on.sample_buf_bytes() <= T * 256 * spp * 12 * 9 // 8, on.sample_buf_bytes()
    nobuf = api.Context(api.Scene(sd), 0)
    nobuf.set_option("fused_tail_blocks", T)
    nobuf.set_option("fused_tail_no_buffer_test", 1)
    img, st = nobuf.render(seeds, api.path_params(spp=spp))
    assert img.tobytes() == ref.tobytes() and st["kernel_launches"] == rst["kernel_launches"] and nobuf.sample_buf_bytes() == 0
    assert all(st[k] == rst[k] for k in COUNTERS) and api.lib().rl_last_error() in (None, b"")


def test_automatic_tail_is_for_the_measured_form_only(built):
    """The automatic choice: a large frame of one diffuse BSDF under area lights, exact numerics, the only path render in flight.  Other forms of the kernel get a tail
    from the options only (same image either way)."""
    W, H = 1920, 1080
    seeds = api.IndependentSampler(4).block_seeds(W, H)
    sd = scenes.cbox(W, H)
    ctx = api.Context(api.Scene(sd), 0)
    _, st_auto = ctx.render(seeds, api.path_params(spp=2))
    assert ctx.sample_buf_bytes() > 0                                   # the headline's form: on
    fast = api.Context(api.Scene(sd), 0)
    a, _ = fast.render(seeds, api.path_params(spp=2, numerics=1))
    assert fast.sample_buf_bytes() == 0                                 # the tolerance build: off ...
    fast.set_option("fused_tail_blocks", 512)
    b, _ = fast.render(seeds, api.path_params(spp=2, numerics=1))
    assert fast.sample_buf_bytes() > 0 and a.tobytes() == b.tobytes()   # ... unless asked for
    meshes = [dataclasses.replace(m, bsdf=scenes.living_room_materials()[1]) if m.name == "TallBox" else m for m in sd.meshes]
    mixed = api.Context(api.Scene(dataclasses.replace(sd, meshes=meshes)), 0)
    a, _ = mixed.render(seeds, api.path_params(spp=2))
    assert mixed.sample_buf_bytes() == 0                                # two BSDF types (the run-time material switch): off
    mixed.set_option("fused_tail_blocks", 512)
    b, _ = mixed.render(seeds, api.path_params(spp=2))
    assert mixed.sample_buf_bytes() > 0 and a.tobytes() == b.tobytes()


def test_full_frame_with_the_automatic_tail_equals_the_oracle(built):
    """The headline frame (1920 x 1080 x 128 spp, per-sample streams, master seed 2) with the options left alone — the automatic tail — against the CRC and the
    counters the CPU oracle's parity build gave for it (tests/golden/bench_crcs.json)."""
    e = json.load(open(os.path.join(GOLDEN, "bench_crcs.json")))["cbox:1920x1080x128:per_sample:seed2"]
    ctx = api.Context(api.Scene(scenes.cbox(1920, 1080)), 0)
    seeds = api.IndependentSampler(2).block_seeds(1920, 1080)
    img, st = ctx.render(seeds, api.path_params(spp=128))
    assert f"{zlib.crc32(img.tobytes()):08x}" == e["crc32"]
    assert (st["camera_samples"], st["vertices"], st["rng_draws"]) == (e["camera_samples"], e["vertices"], e["rng_draws"])
    with ctx.options(fused_tail_blocks=0):
        _, st0 = ctx.render(seeds, api.path_params(spp=128))
    assert st["kernel_launches"] == st0["kernel_launches"] + 1          # the automatic tail was on


def test_forms_without_a_tail_ignore_the_options(built, monkeypatch):
    """cbox + medium, a scene that streams its BVH, reference-order streams and the stratified sampler: the options change neither their launches nor their images —
    the committed golden renders (tests/golden/features.npz) and, for the stratified sampler, the oracle's."""
    from tests.golden.make_golden import feature_cases
    gold = np.load(os.path.join(GOLDEN, "features.npz"))
    cases = feature_cases()

    def both(ctx, seeds, params):
        img0, st0 = ctx.render(seeds, params)
        with ctx.options(fused_tail_blocks=7, fused_tail_split=4):
            img, st = ctx.render(seeds, params)
        assert st["kernel_launches"] == st0["kernel_launches"] and img.tobytes() == img0.tobytes()
        return img

    for name, streaming in (("medium_hg", False), ("reference_order", False), ("mixed_materials", True)):
        sd, _, kw = cases[name]
        if streaming:
            monkeypatch.setenv("RL_FORCE_STREAMING", "1")       # (read when the context is created)
        ctx = api.Context(api.Scene(sd), 0)
        monkeypatch.delenv("RL_FORCE_STREAMING", raising=False)
        np.testing.assert_array_equal(both(ctx, api.IndependentSampler(7).block_seeds(sd.width, sd.height), api.path_params(**kw)), gold[name], err_msg=name)
    sd = scenes.cbox(96, 64)
    seeds = api.IndependentSampler(11).block_seeds(96, 64)
    img = both(api.Context(api.Scene(sd), 0), seeds, api.path_params(spp=4, stream_mode=api.STREAM_STRATIFIED))
    ref = orc.Scene(sd).render(seeds=seeds, spp=4, stream_mode=api.STREAM_STRATIFIED, eval_order=1)
    np.testing.assert_array_equal(img, ref[0] if isinstance(ref, tuple) else ref)
