"""rl_render_point_normal_taylor on the device against tests/pntaylor_restatement.py: the image and all five counters bit for bit.  Frame 24 x 18 (2 x 2
blocks, both edges ragged) at 3 spp: the six strategies x AA on / off x both stream modes in a coloured medium with Henyey-Greenstein g = 0.6 and in the Cornell
box with its isotropic medium, where the two eq phase polynomials are rl_render_point_normal's eq_ex / eq_clamped_ex byte for byte and pn_phase_taylor_ex is
refused; a second area light plus a point light and one floating light quad that most camera rays miss, for the None outcomes, asserted present in the
restatement before the device is asked; a 1 x 1 and a 17 x 1 frame; three shards; the single-pass walk (ref_single_pass) against the parallel form; the BVH
streamed; the CLI and IntegratorPointNormalTaylor; the refused inputs' codes; kernel_launches = 3 in reference order."""
import os
import subprocess

import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import cli
from tests import pn_restatement as P
from tests import pntaylor_restatement as T
from tests.scene_helpers import context as _context

pytestmark = pytest.mark.gpu

W, H, SPP = 24, 18, 3
REF, PER = api.STREAM_REFERENCE_ORDER, api.STREAM_PER_SAMPLE
TR = ("eq_tr_taylor_ex", "eq_clamped_tr_taylor_ex", "pn_tr_taylor_ex")          # the strategies an isotropic medium neither forwards nor refuses
RL_ERR_INVALID_ARGUMENT = -1


def _same(got, want):
    img, st = got
    ref, counters = want[0], want[1]
    assert img.tobytes() == ref.tobytes(), (int((img != ref).any(axis=2).sum()), float(np.nanmax(np.abs(img - ref))))
    assert {k: st[k] for k in T.COUNTERS} == counters


_CTX = {}


def _ctx(name, w=W, h=H, streaming=False):
    """One context per scene, shared by the tests of this file."""
    key = (name, w, h, streaming)
    if key not in _CTX:
        _CTX[key] = _context(T.scene(name, w, h), streaming=streaming)
    return _CTX[key]


@pytest.mark.parametrize("mode", [REF, PER])
@pytest.mark.parametrize("use_aa", [True, False])
@pytest.mark.parametrize("strategy", T.STRATEGIES)
def test_every_strategy_in_the_coloured_medium(built, strategy, use_aa, mode):
    fr, seeds, img, st, det = T.fixture("coloured", strategy, SPP, use_aa, mode)
    assert img.any() and det["took_poly"] > 0
    assert st["rng_draws"] == st["camera_samples"] * (6 if use_aa else 4) + det["some"] and st["vertices"] == det["some"]
    got = _ctx("coloured").render_point_normal_taylor(seeds, strategy, SPP, use_aa, mode)
    _same(got, (img, st))
    assert got[1]["kernel_launches"] == (3 if mode == REF else 2)


@pytest.mark.parametrize("mode", [REF, PER])
@pytest.mark.parametrize("use_aa", [True, False])
@pytest.mark.parametrize("strategy", T.STRATEGIES)
def test_every_strategy_in_the_isotropic_box(built, strategy, use_aa, mode):
    seeds = orc.block_seeds(7, W, H)
    ctx = _ctx("box")
    if strategy == "pn_phase_taylor_ex":                                                     # assert!(g != 0.0): refused before any kernel
        assert _code(ctx.render_point_normal_taylor, seeds, strategy, SPP, use_aa, mode) == api.RL_ERR_UNSUPPORTED
        with pytest.raises(T.Refused) as e:
            T.render(T.frame("box"), seeds, strategy, SPP, use_aa, mode)
        assert e.value.code == api.RL_ERR_UNSUPPORTED
        return
    fr, seeds, img, st, det = T.fixture("box", strategy, SPP, use_aa, mode)
    assert img.any()
    got = ctx.render_point_normal_taylor(seeds, strategy, SPP, use_aa, mode)
    _same(got, (img, st))
    plain = T.forwarded(fr.medium, strategy)
    if plain is None:
        assert got[1]["kernel_launches"] == (3 if mode == REF else 2)
    else:                                                                                    # the bytes of rl_render_point_normal
        assert plain == {"eq_phase_taylor_ex": "eq_ex", "eq_clamped_phase_taylor_ex": "eq_clamped_ex"}[strategy]
        want = ctx.render_point_normal(seeds, plain, SPP, use_aa, mode)
        assert got[0].tobytes() == want[0].tobytes()
        assert all(got[1][k] == want[1][k] for k in T.COUNTERS + ("kernel_launches",))


@pytest.mark.parametrize("strategy", TR)
@pytest.mark.parametrize("name", ["lights", "floating"])
def test_more_lights_and_rays_that_miss(built, name, strategy):
    for mode in (REF, PER):
        fr, seeds, img, st, det = T.fixture(name, strategy, SPP, True, mode)
        if strategy != "eq_tr_taylor_ex":
            assert det["some"] > 0 and det["none"] > 0, "the restatement meets both outcomes of the None test"
        if name == "floating":
            assert det["took_poly"] > 0 and det["took_other"] > 0 and det["branch_mixed"] > 0
            if strategy != "eq_tr_taylor_ex":
                assert det["branch_low"] > 0
            if strategy == "pn_tr_taylor_ex":
                assert det["none_pn"] > 0 and det["none_base"] > 0
        assert st["rng_draws"] == st["camera_samples"] * 6 + det["some"] and st["vertices"] == det["some"]
        _same(_ctx(name).render_point_normal_taylor(seeds, strategy, SPP, True, mode), (img, st))


@pytest.mark.parametrize("strategy", TR)
@pytest.mark.parametrize("size", [(1, 1), (17, 1)])
def test_small_frames(built, size, strategy):
    w, h = size
    for mode in (REF, PER):
        fr, seeds, img, st, det = T.fixture("lights", strategy, SPP, True, mode, w, h)
        _same(_ctx("lights", w, h).render_point_normal_taylor(seeds, strategy, SPP, True, mode), (img, st))


@pytest.mark.parametrize("strategy", T.STRATEGIES)
def test_three_shards_sum_to_the_image(built, strategy):
    fr, seeds, img, st, det = T.fixture("coloured", strategy, SPP)
    ctx = _ctx("coloured")
    total, counters = np.zeros_like(img), {k: 0 for k in T.COUNTERS}
    for i in range(3):
        part = T.fixture("coloured", strategy, SPP, shard_index=i, shard_count=3)
        got = ctx.render_point_normal_taylor(seeds, strategy, SPP, shard_index=i, shard_count=3)
        _same(got, (part[2], part[3]))
        total += got[0]
        for k in T.COUNTERS:
            counters[k] += got[1][k]
    assert total.tobytes() == img.tobytes() and counters == st


@pytest.mark.parametrize("strategy", ["eq_clamped_tr_taylor_ex", "pn_tr_taylor_ex"])
def test_single_pass_equals_the_parallel_form(built, strategy):
    fr, seeds, img, st, det = T.fixture("lights", strategy, SPP)
    ctx = _context(T.scene("lights"))
    parallel = ctx.render_point_normal_taylor(seeds, strategy, SPP)
    ctx.set_option("ref_single_pass", 1)
    single = ctx.render_point_normal_taylor(seeds, strategy, SPP)
    assert parallel[1]["kernel_launches"] == 3 and single[1]["kernel_launches"] == 1
    assert single[0].tobytes() == parallel[0].tobytes() and all(single[1][k] == parallel[1][k] for k in T.COUNTERS)
    _same(single, (img, st))


@pytest.mark.parametrize("strategy", T.STRATEGIES)
def test_streamed_bvh(built, strategy):
    """The kernels of pntaylor_stream.hip: the same bytes with the BVH streamed from memory."""
    for mode in (REF, PER):
        fr, seeds, img, st, det = T.fixture("coloured", strategy, SPP, True, mode)
        _same(_ctx("coloured", streaming=True).render_point_normal_taylor(seeds, strategy, SPP, True, mode), (img, st))


# ---- refusals
def _code(fn, *a, **kw):
    with pytest.raises(api.RustlightError) as e:
        fn(*a, **kw)
    return e.value.code


def test_refused_scenes(built):
    seeds = orc.block_seeds(0, 16, 16)
    assert _code(_context(scenes.cbox(16, 16)).render_point_normal_taylor, seeds) == api.RL_ERR_UNSUPPORTED                     # no medium
    sd = scenes.cbox_medium(16, 16, 1.0); sd.use_ats = True
    assert _code(_context(sd).render_point_normal_taylor, seeds) == api.RL_ERR_UNSUPPORTED                                      # the light tree
    sd = scenes.cbox_other_lights(16, 16, point=False, directional=True, environment=False)
    sd.medium = scenes.cbox_medium(16, 16, 1.0).medium
    assert _code(_context(sd).render_point_normal_taylor, seeds) == api.RL_ERR_UNSUPPORTED                                      # a directional light
    sd = scenes.cbox_medium(16, 16, 1.0); sd.meshes[-1].emission = None
    assert _code(_context(sd).render_point_normal_taylor, seeds) == api.RL_ERR_NO_EMITTER
    # Henyey-Greenstein with g = 0 is still g = 0 for pn_phase_taylor_ex
    sd = scenes.cbox(16, 16, scenes.Medium((0.0,) * 3, (1.0,) * 3, scenes.PHASE_HG, 0.0))
    assert _code(_context(sd).render_point_normal_taylor, seeds, "pn_phase_taylor_ex") == api.RL_ERR_UNSUPPORTED


def test_refused_arguments(built):
    ctx = _ctx("box", 16, 16)
    seeds = orc.block_seeds(0, 16, 16)
    for strategy in (-1, 6):
        assert _code(ctx.render_point_normal_taylor, seeds, strategy) == RL_ERR_INVALID_ARGUMENT, strategy
    for name in ("pn_best_ex", "eq_ex"):
        with pytest.raises(ValueError):
            ctx.render_point_normal_taylor(seeds, name)
    for kw, code in (({"spp": 0}, RL_ERR_INVALID_ARGUMENT), ({"shard_index": 2, "shard_count": 2}, RL_ERR_INVALID_ARGUMENT),
                     ({"stream_mode": api.STREAM_STRATIFIED}, api.RL_ERR_UNSUPPORTED), ({"stream_mode": 3}, RL_ERR_INVALID_ARGUMENT)):
        assert _code(ctx.render_point_normal_taylor, seeds, "eq_tr_taylor_ex", **kw) == code, kw
    assert _code(ctx.render_point_normal_taylor, seeds[:0]) == RL_ERR_INVALID_ARGUMENT


# ---- mirrors
@pytest.mark.parametrize("strategy,use_aa,mode", [("pn_phase_taylor_ex", True, REF), ("eq_clamped_phase_taylor_ex", False, PER), ("eq_tr_taylor_ex", True, REF)])
def test_integrator_compute(built, strategy, use_aa, mode):
    sd = T.scene("coloured")
    integ = api.IntegratorPointNormalTaylor(strategy, use_aa, mode)
    img = integ.compute(api.IndependentSampler(9), api.Scene(sd), 2)
    ref = T.compute(sd, 9, strategy, 2, use_aa, mode)
    assert img.any() and img.tobytes() == ref["image"].tobytes()
    for k in T.COUNTERS:
        assert integ.last_stats[k] == ref["stats"][k], k


def _run_cli(tmp_path, *args):
    scn = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "cbox.pbrt")
    out = str(tmp_path / "pntaylor.pfm")
    r = subprocess.run([cli.EXE, scn, *args[0], "-r", "independent:7", "-o", out, "point-normal-taylor", *args[1]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return scn, api.load_pfm(out)


def test_cli_writes_the_restatements_bytes(built, tmp_path):
    """`data/cbox.pbrt -n 4 -s 0.0625 -m 1.0 -r independent:7 point-normal-taylor -s pn_tr_taylor_ex` through the C++ mirror (integrator.hpp:
    IntegratorPointNormalTaylor::compute): the restatement's image of the same box at 32 x 32."""
    scn, img = _run_cli(tmp_path, ("-n", "4", "-s", "0.0625", "-m", "1.0"), ("-s", "pn_tr_taylor_ex"))
    assert img.shape == (32, 32, 3)
    ref = T.compute(scenes.cbox_medium(32, 32, 1.0), 7, "pn_tr_taylor_ex", 4)
    assert ref["image"].any() and np.abs(img).tobytes() == np.abs(ref["image"]).tobytes()      # (save_pfm writes |value|)


def test_cli_renders_what_the_api_renders(built, tmp_path):
    """The default strategy at 32 x 32, with AA off on per-sample streams: the bytes of the Python mirror; and pn_phase_taylor_ex in the isotropic medium
    exits 2."""
    scn, img = _run_cli(tmp_path, ("-n", "2", "-s", "0.0625", "-m", "1.0", "--stream-mode", "per-sample"), ("-z",))
    ref = T.compute(scenes.cbox_medium(32, 32, 1.0), 7, "eq_tr_taylor_ex", 2, False, PER)
    assert ref["image"].any() and np.abs(img).tobytes() == np.abs(ref["image"]).tobytes()
    r = subprocess.run([cli.EXE, scn, "-n", "1", "-s", "0.0625", "-m", "1.0", "-o", str(tmp_path / "x.pfm"), "point-normal-taylor", "-s", "pn_phase_taylor_ex"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "pn_phase_taylor_ex" in r.stderr, (r.returncode, r.stderr)
