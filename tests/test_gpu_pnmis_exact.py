"""rl_render_point_normal_mis on the device against tests/pnmis_restatement.py: the image and all five counters bit for bit.  Frame 24 x 18 (2 x 2 blocks,
both edges ragged) at 3 spp: every family x AA on / off x both stream modes in the Cornell box with its medium; then a coloured medium with
Henyey-Greenstein g = 0.6, a second area light plus a point light (the kept departure: the point light takes its draws and adds nothing), one floating light
quad that most camera rays miss (the unbounded arms); a 1 x 1 and a 17 x 1 frame; three shards; the single-pass walk (ref_single_pass) against the parallel
form for a constant-count and a data-dependent family; the BVH streamed; the two names of every family; the CLI and IntegratorPointNormalMis; the refused
inputs' codes.  On `lights` and `floating` the restatement counts both outcomes of the None test, asserted before the device is asked."""
import copy
import os
import subprocess

import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import cli
from tests import pn_restatement as P
from tests import pnmis_restatement as M
from tests.scene_helpers import context as _context

pytestmark = pytest.mark.gpu

W, H, SPP = 24, 18, 3
REF, PER = api.STREAM_REFERENCE_ORDER, api.STREAM_PER_SAMPLE
ONE_NAME = ("tr_ex", "eq_phase", "eq_clamped_ex", "pn_ex")          # one name of each family
RL_ERR_INVALID_ARGUMENT = -1


def _same(got, want):
    img, st = got
    ref, counters = want[0], want[1]
    assert img.tobytes() == ref.tobytes(), (int((img != ref).any(axis=2).sum()), float(np.nanmax(np.abs(img - ref))))
    assert {k: st[k] for k in M.COUNTERS} == counters


_CTX = {}


def _ctx(name, w=W, h=H, streaming=False):
    """One context per scene, shared by the tests of this file."""
    key = (name, w, h, streaming)
    if key not in _CTX:
        _CTX[key] = _context(M.scene(name, w, h), streaming=streaming)
    return _CTX[key]


@pytest.mark.parametrize("mode", [REF, PER])
@pytest.mark.parametrize("use_aa", [True, False])
@pytest.mark.parametrize("strategy", ONE_NAME)
def test_every_family_in_the_box(built, strategy, use_aa, mode):
    fr, seeds, img, st, det = M.fixture("box", strategy, SPP, use_aa, mode)
    assert img.any()
    got = _ctx("box").render_point_normal_mis(seeds, strategy, SPP, use_aa, mode)
    _same(got, (img, st))
    assert got[1]["kernel_launches"] == (3 if mode == REF and M.draws_per_sample(strategy) is None else 2)


@pytest.mark.parametrize("strategy", ONE_NAME)
@pytest.mark.parametrize("name", ["coloured", "lights", "floating"])
def test_other_media_lights_and_rays_that_miss(built, name, strategy):
    for mode in (REF, PER):
        fr, seeds, img, st, det = M.fixture(name, strategy, SPP, True, mode)
        if M.draws_per_sample(strategy) is None and name != "coloured":
            assert det["some"] > 0 and det["none"] > 0, "the restatement meets both outcomes of the None test"
            assert st["rng_draws"] == st["camera_samples"] * 10 + det["some"] and st["vertices"] == det["some"]
        _same(_ctx(name).render_point_normal_mis(seeds, strategy, SPP, True, mode), (img, st))


def test_the_point_light_alone_adds_nothing(built):
    """The kept departure: every explicit technique is zero on the point light's zero normal and no phase ray hits it."""
    sd = M.scene("box")
    for m in sd.meshes:
        m.emission = None
    sd.lights.append(copy.deepcopy(P.POINT_LIGHT))
    fr, seeds, ctx = M.Frame(sd), orc.block_seeds(5, W, H), _context(sd)
    for strategy in ONE_NAME:
        img, st, det = M.render(fr, seeds, strategy, 2)
        assert not img.any() and st["shadow_rays"] == 0
        _same(ctx.render_point_normal_mis(seeds, strategy, 2), (img, st))


@pytest.mark.parametrize("strategy", ONE_NAME)
@pytest.mark.parametrize("size", [(1, 1), (17, 1)])
def test_small_frames(built, size, strategy):
    w, h = size
    for mode in (REF, PER):
        fr, seeds, img, st, det = M.fixture("lights", strategy, SPP, True, mode, w, h)
        _same(_ctx("lights", w, h).render_point_normal_mis(seeds, strategy, SPP, True, mode), (img, st))


@pytest.mark.parametrize("strategy", ONE_NAME)
def test_three_shards_sum_to_the_image(built, strategy):
    fr, seeds, img, st, det = M.fixture("lights", strategy, SPP)
    ctx = _ctx("lights")
    total, counters = np.zeros_like(img), {k: 0 for k in M.COUNTERS}
    for i in range(3):
        part = M.fixture("lights", strategy, SPP, shard_index=i, shard_count=3)
        got = ctx.render_point_normal_mis(seeds, strategy, SPP, shard_index=i, shard_count=3)
        _same(got, (part[2], part[3]))
        total += got[0]
        for k in M.COUNTERS:
            counters[k] += got[1][k]
    assert total.tobytes() == img.tobytes() and counters == st


@pytest.mark.parametrize("strategy", ["eq_ex", "pn_ex"])       # a constant count (jump-ahead) and a data-dependent one (chain pass)
def test_single_pass_equals_the_parallel_form(built, strategy):
    fr, seeds, img, st, det = M.fixture("lights", strategy, SPP)
    ctx = _context(M.scene("lights"))
    parallel = ctx.render_point_normal_mis(seeds, strategy, SPP)
    ctx.set_option("ref_single_pass", 1)
    single = ctx.render_point_normal_mis(seeds, strategy, SPP)
    assert parallel[1]["kernel_launches"] > 1 and single[1]["kernel_launches"] == 1
    assert single[0].tobytes() == parallel[0].tobytes() and all(single[1][k] == parallel[1][k] for k in M.COUNTERS)
    _same(single, (img, st))


@pytest.mark.parametrize("strategy", ONE_NAME)
def test_streamed_bvh(built, strategy):
    """The kernels of pnmis_stream.hip: the same bytes with the BVH streamed from memory."""
    for mode in (REF, PER):
        fr, seeds, img, st, det = M.fixture("lights", strategy, SPP, True, mode)
        _same(_ctx("lights", streaming=True).render_point_normal_mis(seeds, strategy, SPP, True, mode), (img, st))


@pytest.mark.parametrize("pair", [("tr_ex", "tr_phase"), ("eq_ex", "eq_phase"), ("eq_clamped_ex", "eq_clamped_phase")])
def test_the_two_names_of_a_family_give_equal_bytes(built, pair):
    seeds = orc.block_seeds(7, W, H)
    a = _ctx("coloured").render_point_normal_mis(seeds, pair[0], SPP)
    b = _ctx("coloured").render_point_normal_mis(seeds, pair[1], SPP)
    assert a[0].any() and a[0].tobytes() == b[0].tobytes() and all(a[1][k] == b[1][k] for k in M.COUNTERS)


# ---- refusals
def _code(fn, *a, **kw):
    with pytest.raises(api.RustlightError) as e:
        fn(*a, **kw)
    return e.value.code


def test_refused_scenes(built):
    seeds = orc.block_seeds(0, 16, 16)
    assert _code(_context(scenes.cbox(16, 16)).render_point_normal_mis, seeds) == api.RL_ERR_UNSUPPORTED                        # no medium
    sd = scenes.cbox_medium(16, 16, 1.0); sd.use_ats = True
    assert _code(_context(sd).render_point_normal_mis, seeds) == api.RL_ERR_UNSUPPORTED                                         # the light tree
    sd = scenes.cbox_other_lights(16, 16, point=False, directional=True, environment=False)
    sd.medium = scenes.cbox_medium(16, 16, 1.0).medium
    assert _code(_context(sd).render_point_normal_mis, seeds) == api.RL_ERR_UNSUPPORTED                                         # a directional light
    sd = scenes.cbox_other_lights(16, 16, point=False, directional=False, environment=True)
    sd.medium = scenes.cbox_medium(16, 16, 1.0).medium
    assert _code(_context, sd) == api.RL_ERR_UNSUPPORTED                      # an environment emitter: with a medium the context itself refuses it
    sd = scenes.cbox_medium(16, 16, 1.0); sd.meshes[-1].emission = None
    assert _code(_context(sd).render_point_normal_mis, seeds) == api.RL_ERR_NO_EMITTER


def test_refused_arguments(built):
    ctx = _ctx("box", 16, 16)
    seeds = orc.block_seeds(0, 16, 16)
    for strategy in (-1, 7):
        assert _code(ctx.render_point_normal_mis, seeds, strategy) == RL_ERR_INVALID_ARGUMENT, strategy
    with pytest.raises(ValueError):
        ctx.render_point_normal_mis(seeds, "pn_best_ex")
    for kw, code in (({"spp": 0}, RL_ERR_INVALID_ARGUMENT), ({"shard_index": 2, "shard_count": 2}, RL_ERR_INVALID_ARGUMENT),
                     ({"stream_mode": api.STREAM_STRATIFIED}, api.RL_ERR_UNSUPPORTED), ({"stream_mode": 3}, RL_ERR_INVALID_ARGUMENT)):
        assert _code(ctx.render_point_normal_mis, seeds, "tr_ex", **kw) == code, kw
    assert _code(ctx.render_point_normal_mis, seeds[:0]) == RL_ERR_INVALID_ARGUMENT
    # the jump-ahead's reach, 256 * spp * D <= 2^32 - 1 with D = 9 for tr and 10 for eq: refused before any kernel
    for strategy, d in (("tr_phase", 9), ("eq_ex", 10)):
        spp = (1 << 32) // (256 * d) + 1
        assert 256 * spp * d > 2 ** 32 - 1
        assert _code(ctx.render_point_normal_mis, seeds, strategy, spp) == api.RL_ERR_UNSUPPORTED


# ---- mirrors
@pytest.mark.parametrize("strategy,use_aa,mode", [("pn_ex", True, REF), ("eq_clamped_phase", False, PER), ("tr_ex", True, REF), ("eq_ex", True, REF)])
def test_integrator_compute(built, strategy, use_aa, mode):
    sd = M.scene("lights")
    integ = api.IntegratorPointNormalMis(strategy, use_aa, mode)
    img = integ.compute(api.IndependentSampler(9), api.Scene(sd), 2)
    ref = M.compute(sd, 9, strategy, 2, use_aa, mode)
    assert img.any() and img.tobytes() == ref["image"].tobytes()
    for k in M.COUNTERS:
        assert integ.last_stats[k] == ref["stats"][k], k


def _run_cli(tmp_path, *args):
    scn = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "cbox.pbrt")
    out = str(tmp_path / "pnmis.pfm")
    r = subprocess.run([cli.EXE, scn, *args[0], "-m", "1.0", "-r", "independent:7", "-o", out, "point-normal-mis", *args[1]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return scn, api.load_pfm(out)


def test_cli_writes_the_restatements_bytes(built, tmp_path):
    """`data/cbox.pbrt -n 4 -s 0.0625 -m 1.0 -r independent:7 point-normal-mis -s pn_ex` through the C++ mirror (integrator.hpp:
    IntegratorPointNormalMis::compute): the restatement's image of the same box at 32 x 32."""
    scn, img = _run_cli(tmp_path, ("-n", "4", "-s", "0.0625"), ("-s", "pn_ex"))
    assert img.shape == (32, 32, 3)
    ref = M.compute(scenes.cbox_medium(32, 32, 1.0), 7, "pn_ex", 4)
    assert ref["image"].any() and np.abs(img).tobytes() == np.abs(ref["image"]).tobytes()      # (save_pfm writes |value|)


def test_cli_renders_what_the_api_renders(built, tmp_path):
    """The default strategy at the scene's own 512 x 512, with AA off on per-sample streams: the bytes of the Python mirror."""
    scn, img = _run_cli(tmp_path, ("-n", "2", "--stream-mode", "per-sample"), ("-z",))
    scene = api.Scene.load(scn)
    scene.set_medium((0.0,) * 3, (1.0,) * 3)
    want = api.IntegratorPointNormalMis("tr_ex", False, PER).compute(api.IndependentSampler(7), scene, 2)
    assert img.shape == want.shape and want.any()
    np.testing.assert_array_equal(img, np.abs(want))
