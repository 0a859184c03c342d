"""rl_render_point_normal on the device against tests/pn_restatement.py: the image and all five counters bit for bit.  Frame 24 x 18 (2 x 2 blocks, both
edges ragged), the Cornell box with its medium, every strategy x AA on / off x both stream modes at 3 spp; then, on pn_ex, eq_clamped_phase and tr_ex, a
coloured medium with Henyey-Greenstein g = 0.6, a second area light plus a point light, one floating light quad that most rays miss, a 1 x 1 and a 17 x 1
frame, three shards, and the single-pass walk (ref_single_pass) against the parallel form; the BVH streamed instead of staged in LDS; the CLI and the
IntegratorPointNormal class; the refused inputs' codes.  The restatement counts both outcomes of the None test in the cases that are there for it, asserted
before the device is asked."""
import os
import subprocess

import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import cli
from tests import pn_restatement as P
from tests.scene_helpers import context as _context

pytestmark = pytest.mark.gpu

W, H, SPP = 24, 18, 3
REF, PER = api.STREAM_REFERENCE_ORDER, api.STREAM_PER_SAMPLE
THREE = ("pn_ex", "eq_clamped_phase", "tr_ex")
RL_ERR_INVALID_ARGUMENT = -1


def _same(got, want):
    img, st = got
    ref, counters = want[0], want[1]
    assert img.tobytes() == ref.tobytes(), (int((img != ref).any(axis=2).sum()), float(np.abs(img - ref).max()))
    assert {k: st[k] for k in P.COUNTERS} == counters


_CTX = {}


def _ctx(name, w=W, h=H, streaming=False):
    """One context per scene, shared by the tests of this file."""
    key = (name, w, h, streaming)
    if key not in _CTX:
        _CTX[key] = _context(P.scene(name, w, h), streaming=streaming)
    return _CTX[key]


@pytest.mark.parametrize("mode", [REF, PER])
@pytest.mark.parametrize("use_aa", [True, False])
@pytest.mark.parametrize("strategy", P.STRATEGIES)
def test_every_strategy_in_the_box(built, strategy, use_aa, mode):
    fr, seeds, img, st, det = P.fixture("box", strategy, SPP, use_aa, mode)
    assert img.any() or strategy == "tr_phase"                 # (a free path from the camera rarely ends where the phase ray finds the light)
    got = _ctx("box").render_point_normal(seeds, strategy, SPP, use_aa, mode)
    _same(got, (img, st))
    assert got[1]["kernel_launches"] == (3 if mode == REF and P.may_fail(strategy) else 2)


@pytest.mark.parametrize("strategy", THREE)
@pytest.mark.parametrize("name", ["coloured", "lights", "floating"])
def test_other_media_lights_and_rays_that_miss(built, name, strategy):
    for mode in (REF, PER):
        fr, seeds, img, st, det = P.fixture(name, strategy, SPP, True, mode)
        if P.may_fail(strategy) and name != "coloured":
            assert det["some"] > 0 and det["none"] > 0, "the restatement meets both outcomes of the None test"
            assert st["rng_draws"] == st["camera_samples"] * 6 + det["some"] * (3 if P.is_phase(strategy) else 1)
        _same(_ctx(name).render_point_normal(seeds, strategy, SPP, True, mode), (img, st))


def test_most_rays_of_the_floating_light_miss(built):
    px, py, o, d, tfar = P.camera_rays(P.frame("floating"), orc.block_seeds(7, W, H), "tr_ex", 1)
    assert 0 < (tfar < P.F32_MAX).mean() < 0.2


@pytest.mark.parametrize("strategy", THREE)
@pytest.mark.parametrize("size", [(1, 1), (17, 1)])
def test_small_frames(built, size, strategy):
    w, h = size
    for mode in (REF, PER):
        fr, seeds, img, st, det = P.fixture("lights", strategy, SPP, True, mode, w, h)
        _same(_ctx("lights", w, h).render_point_normal(seeds, strategy, SPP, True, mode), (img, st))


@pytest.mark.parametrize("strategy", THREE)
def test_three_shards_sum_to_the_image(built, strategy):
    fr, seeds, img, st, det = P.fixture("lights", strategy, SPP)
    ctx = _ctx("lights")
    total, counters = np.zeros_like(img), {k: 0 for k in P.COUNTERS}
    for i in range(3):
        part = P.fixture("lights", strategy, SPP, shard_index=i, shard_count=3)
        got = ctx.render_point_normal(seeds, strategy, SPP, shard_index=i, shard_count=3)
        _same(got, (part[2], part[3]))
        total += got[0]
        for k in P.COUNTERS:
            counters[k] += got[1][k]
    assert total.tobytes() == img.tobytes() and counters == st


@pytest.mark.parametrize("strategy", ["eq_phase", "pn_ex"])       # a constant count (jump-ahead) and a data-dependent one (chain pass)
def test_single_pass_equals_the_parallel_form(built, strategy):
    fr, seeds, img, st, det = P.fixture("lights", strategy, SPP)
    ctx = _context(P.scene("lights"))
    parallel = ctx.render_point_normal(seeds, strategy, SPP)
    ctx.set_option("ref_single_pass", 1)
    single = ctx.render_point_normal(seeds, strategy, SPP)
    assert parallel[1]["kernel_launches"] > 1 and single[1]["kernel_launches"] == 1
    assert single[0].tobytes() == parallel[0].tobytes() and all(single[1][k] == parallel[1][k] for k in P.COUNTERS)
    _same(single, (img, st))


@pytest.mark.parametrize("strategy", P.STRATEGIES)
def test_streamed_bvh(built, strategy):
    """The kernels of pn_stream.hip: the same bytes with the BVH streamed from memory."""
    for mode in (REF, PER):
        fr, seeds, img, st, det = P.fixture("lights", strategy, SPP, True, mode)
        _same(_ctx("lights", streaming=True).render_point_normal(seeds, strategy, SPP, True, mode), (img, st))


# ---- refusals
def _code(fn, *a, **kw):
    with pytest.raises(api.RustlightError) as e:
        fn(*a, **kw)
    return e.value.code


def test_refused_scenes(built):
    seeds = orc.block_seeds(0, 16, 16)
    assert _code(_context(scenes.cbox(16, 16)).render_point_normal, seeds) == api.RL_ERR_UNSUPPORTED                            # no medium
    sd = scenes.cbox_medium(16, 16, 1.0); sd.use_ats = True
    assert _code(_context(sd).render_point_normal, seeds) == api.RL_ERR_UNSUPPORTED                                             # the light tree
    sd = scenes.cbox_other_lights(16, 16, point=False, directional=True, environment=False)
    sd.medium = scenes.cbox_medium(16, 16, 1.0).medium
    assert _code(_context(sd).render_point_normal, seeds) == api.RL_ERR_UNSUPPORTED                                             # a directional light
    sd = scenes.cbox_medium(16, 16, 1.0); sd.meshes[-1].emission = None
    assert _code(_context(sd).render_point_normal, seeds) == api.RL_ERR_NO_EMITTER


def test_refused_arguments(built):
    ctx = _ctx("box", 16, 16)
    seeds = orc.block_seeds(0, 16, 16)
    for strategy in (-1, 7):
        assert _code(ctx.render_point_normal, seeds, strategy) == RL_ERR_INVALID_ARGUMENT, strategy
    with pytest.raises(ValueError):
        ctx.render_point_normal(seeds, "pn_best_ex")
    for kw, code in (({"spp": 0}, RL_ERR_INVALID_ARGUMENT), ({"shard_index": 2, "shard_count": 2}, RL_ERR_INVALID_ARGUMENT),
                     ({"stream_mode": api.STREAM_STRATIFIED}, api.RL_ERR_UNSUPPORTED), ({"stream_mode": 3}, RL_ERR_INVALID_ARGUMENT)):
        assert _code(ctx.render_point_normal, seeds, "tr_ex", **kw) == code, kw
    assert _code(ctx.render_point_normal, seeds[:0]) == RL_ERR_INVALID_ARGUMENT
    # the jump-ahead's reach, 256 * spp * D <= 2^32 - 1 with D = 9 for eq_phase: refused before any kernel
    spp = (1 << 32) // (256 * 9) + 1
    assert 256 * spp * 9 > 2 ** 32 - 1
    assert _code(ctx.render_point_normal, seeds, "eq_phase", spp) == api.RL_ERR_UNSUPPORTED


# ---- mirrors
@pytest.mark.parametrize("strategy,use_aa,mode", [("pn_ex", True, REF), ("eq_clamped_phase", False, PER), ("tr_ex", True, REF)])
def test_integrator_compute(built, strategy, use_aa, mode):
    sd = P.scene("lights")
    integ = api.IntegratorPointNormal(strategy, use_aa, mode)
    img = integ.compute(api.IndependentSampler(9), api.Scene(sd), 2)
    ref = P.compute(sd, 9, strategy, 2, use_aa, mode)
    assert img.any() and img.tobytes() == ref["image"].tobytes()
    for k in P.COUNTERS:
        assert integ.last_stats[k] == ref["stats"][k], k


def _run_cli(tmp_path, *args):
    scn = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "cbox.pbrt")
    out = str(tmp_path / "pn.pfm")
    r = subprocess.run([cli.EXE, scn, *args[0], "-m", "1.0", "-r", "independent:7", "-o", out, "point-normal", *args[1]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return scn, api.load_pfm(out)


def test_cli_writes_the_restatements_bytes(built, tmp_path):
    """`data/cbox.pbrt -n 4 -s 0.0625 -m 1.0 -r independent:7 point-normal -s pn_ex` through the C++ mirror (integrator.hpp: IntegratorPointNormal::compute):
    the restatement's image of the same box at 32 x 32."""
    scn, img = _run_cli(tmp_path, ("-n", "4", "-s", "0.0625"), ("-s", "pn_ex"))
    assert img.shape == (32, 32, 3)
    ref = P.compute(scenes.cbox_medium(32, 32, 1.0), 7, "pn_ex", 4)
    assert ref["image"].any() and np.abs(img).tobytes() == np.abs(ref["image"]).tobytes()      # (save_pfm writes |value|)


def test_cli_renders_what_the_api_renders(built, tmp_path):
    """The same line at the scene's own 512 x 512, with AA off on per-sample streams: the bytes of the Python mirror."""
    exe_args = (("-n", "4", "--stream-mode", "per-sample"), ("-s", "eq_clamped_ex", "-z"))
    scn, img = _run_cli(tmp_path, *exe_args)
    scene = api.Scene.load(scn)
    scene.set_medium((0.0,) * 3, (1.0,) * 3)
    want = api.IntegratorPointNormal("eq_clamped_ex", False, PER).compute(api.IndependentSampler(7), scene, 4)
    assert img.shape == want.shape and want.any()
    np.testing.assert_array_equal(img, np.abs(want))
