"""rl_render_point_normal_ats on the device against tests/pnats_restatement.py: the image and all five counters bit for bit.  Frame 24 x 18 (2 x 2 blocks,
both edges ragged), and one 16 x 16 frame at 1 spp with AA off.  Scene lights8: the Cornell box with its medium and eight small emissive quads of different
power, colour and orientation (16 proxies, tree depth 5) — one faces the back wall, one lies below the camera's horizon (no clamped or point-normal sampler
for the rays that rise), one has HSV emission — and the box with its single light (two proxies).  The seven plain strategies x both stream modes x spp 2 with AA
and spp 3 without x the scene staged in LDS and streamed, two shards of three; the six Taylor names on lights8 in the coloured Henyey-Greenstein medium;
tr_phase's identity with `point-normal -s tr_phase` on the scene without the tree; the refusals' codes; the single-pass walk; the CLI and
IntegratorPointNormalAts."""
import os
import subprocess

import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import cli
from tests import pn_restatement as P
from tests import pnats_restatement as A
from tests.scene_helpers import context as _context

pytestmark = pytest.mark.gpu

W, H = 24, 18
REF, PER = api.STREAM_REFERENCE_ORDER, api.STREAM_PER_SAMPLE
RL_ERR_INVALID_ARGUMENT = -1
CASES = [(2, True), (3, False)]                    # spp, AA


def _same(got, want):
    img, st = got
    ref, counters = want[0], want[1]
    assert img.tobytes() == ref.tobytes(), (int((img != ref).any(axis=2).sum()), float(np.nanmax(np.abs(img - ref))))
    assert {k: st[k] for k in P.COUNTERS} == counters


_CTX = {}


def _ctx(name, w=W, h=H, streaming=False):
    """One context per scene, shared by the tests of this file."""
    key = (name, w, h, streaming)
    if key not in _CTX:
        _CTX[key] = _context(A.scene(name, w, h), streaming=streaming)
    return _CTX[key]


def _expected_draws(strategy, st, det, use_aa):
    aa = 2 if use_aa else 0
    d = A.draws_per_sample(strategy, use_aa)
    if d is not None:
        return st["camera_samples"] * d
    behind = 3 if strategy == "eq_clamped_phase" else 1
    return st["camera_samples"] * (aa + 3) + det["some"] * behind


@pytest.mark.parametrize("mode", [REF, PER])
@pytest.mark.parametrize("spp,use_aa", CASES)
@pytest.mark.parametrize("strategy", api.PN_STRATEGIES)
def test_every_plain_strategy_on_lights8(built, strategy, spp, use_aa, mode):
    fr, seeds, img, st, det = A.fixture("lights8", strategy, spp, use_aa, mode)
    assert (img.any() or strategy == "tr_phase") and st["rng_draws"] == _expected_draws(strategy, st, det, use_aa)
    if P.may_fail(strategy):
        assert det["some"] > 0 and det["none"] > 0, "the restatement meets both outcomes of the None test"
    for streaming in (False, True):
        got = _ctx("lights8", streaming=streaming).render_point_normal_ats(seeds, strategy, spp, use_aa, mode)
        _same(got, (img, st))
        assert got[1]["kernel_launches"] == ((3 if A.draws_per_sample(strategy) is None else 2) if mode == REF else 2)


@pytest.mark.parametrize("strategy", api.PN_STRATEGIES)
def test_the_box_with_its_single_light(built, strategy):
    """Two proxies: the shallowest tree, one branch."""
    fr, seeds, img, st, det = A.fixture("box", strategy, 3)
    assert fr.tree.n == 3 and (img.any() or strategy == "tr_phase")      # (three phase rays per pixel seldom find the light)
    for streaming in (False, True):
        _same(_ctx("box", streaming=streaming).render_point_normal_ats(seeds, strategy, 3), (img, st))


@pytest.mark.parametrize("strategy", api.PN_STRATEGIES)
def test_two_shards_of_three(built, strategy):
    fr, seeds, img, st, det = A.fixture("lights8", strategy, 2)
    for i in (1, 2):
        part = A.fixture("lights8", strategy, 2, shard_index=i, shard_count=3)
        _same(_ctx("lights8").render_point_normal_ats(seeds, strategy, 2, shard_index=i, shard_count=3), (part[2], part[3]))
        own = part[2].any(axis=2)
        assert np.array_equal(part[2][own], img[own])


@pytest.mark.parametrize("mode", [REF, PER])
@pytest.mark.parametrize("strategy", api.PN_TAYLOR_STRATEGIES)
def test_the_taylor_names_in_the_coloured_medium(built, strategy, mode):
    fr, seeds, img, st, det = A.fixture("lights8_hg", strategy, 2, True, mode)
    assert img.any() and det["took_poly"] > 0
    assert st["rng_draws"] == st["camera_samples"] * 5 + det["some"] and st["vertices"] == det["some"]
    for streaming in (False, True):
        got = _ctx("lights8_hg", streaming=streaming).render_point_normal_ats(seeds, strategy, 2, True, mode)
        _same(got, (img, st))
        assert got[1]["kernel_launches"] == (3 if mode == REF else 2)


@pytest.mark.parametrize("strategy", ["eq_phase_taylor_ex", "eq_clamped_phase_taylor_ex", "pn_phase_taylor_ex"])
def test_the_phase_polynomials_in_the_isotropic_medium(built, strategy):
    """The two eq names are the plain strategy over the tree, byte for byte; pn_phase_taylor_ex is refused (assert!(g != 0.0))."""
    seeds = orc.block_seeds(7, W, H)
    ctx = _ctx("lights8")
    if strategy == "pn_phase_taylor_ex":
        assert _code(ctx.render_point_normal_ats, seeds, strategy, 2) == api.RL_ERR_UNSUPPORTED
        with pytest.raises(A.Refused):
            A.render(A.frame("lights8"), seeds, strategy, 2)
        return
    plain = {"eq_phase_taylor_ex": "eq_ex", "eq_clamped_phase_taylor_ex": "eq_clamped_ex"}[strategy]
    fr, seeds, img, st, det = A.fixture("lights8", plain, 2)
    got = ctx.render_point_normal_ats(seeds, strategy, 2)
    _same(got, (img, st))
    assert A.render(fr, seeds, strategy, 2)[0].tobytes() == img.tobytes()


def test_one_sample_per_pixel_without_aa_on_one_block(built):
    for strategy in ("eq_ex", "tr_ex", "pn_ex", "pn_tr_taylor_ex"):
        fr, seeds, img, st, det = A.fixture("lights8", strategy, 1, False, REF, 16, 16)
        _same(_ctx("lights8", 16, 16).render_point_normal_ats(seeds, strategy, 1, False), (img, st))


def test_tr_phase_is_point_normals_tr_phase_without_the_tree(built):
    """tr_phase takes no emitter sample: the bytes `point-normal -s tr_phase` gives on the same scene built without the tree."""
    seeds = orc.block_seeds(7, W, H)
    for mode in (REF, PER):
        got = _ctx("lights8").render_point_normal_ats(seeds, "tr_phase", 3, True, mode)
        want = _context(A.lights(8, W, H, use_ats=False)).render_point_normal(seeds, "tr_phase", 3, True, mode)
        assert got[0].tobytes() == want[0].tobytes() and all(got[1][k] == want[1][k] for k in P.COUNTERS)


@pytest.mark.parametrize("strategy", ["eq_clamped_ex", "pn_tr_taylor_ex"])
def test_single_pass_equals_the_parallel_form(built, strategy):
    fr, seeds, img, st, det = A.fixture("lights8", strategy, 2)
    ctx = _context(A.scene("lights8"))
    parallel = ctx.render_point_normal_ats(seeds, strategy, 2)
    ctx.set_option("ref_single_pass", 1)
    single = ctx.render_point_normal_ats(seeds, strategy, 2)
    assert parallel[1]["kernel_launches"] == 3 and single[1]["kernel_launches"] == 1
    assert single[0].tobytes() == parallel[0].tobytes() and all(single[1][k] == parallel[1][k] for k in P.COUNTERS)
    _same(single, (img, st))


# ---- refusals
def _code(fn, *a, **kw):
    with pytest.raises(api.RustlightError) as e:
        fn(*a, **kw)
    return e.value.code


def test_refused_scenes(built):
    seeds = orc.block_seeds(0, 16, 16)
    assert _code(_context(scenes.cbox_medium(16, 16, 1.0)).render_point_normal_ats, seeds) == api.RL_ERR_UNSUPPORTED            # no tree in the scene
    sd = scenes.cbox(16, 16); sd.use_ats = True
    assert _code(_context(sd).render_point_normal_ats, seeds) == api.RL_ERR_UNSUPPORTED                                         # no medium
    sd = scenes.cbox_medium(16, 16, 1.0); sd.lights.append(dict(P.POINT_LIGHT))
    assert _code(_context(sd).render_point_normal_ats, seeds) == api.RL_ERR_UNSUPPORTED                                         # a point light
    with pytest.raises(A.Refused) as e:
        A.Frame(sd)
    assert e.value.code == api.RL_ERR_UNSUPPORTED
    sd = scenes.cbox_other_lights(16, 16, point=False, directional=True, environment=False)
    sd.medium = scenes.cbox_medium(16, 16, 1.0).medium
    assert _code(_context(sd).render_point_normal_ats, seeds) == api.RL_ERR_UNSUPPORTED                                         # a directional light


def test_refused_arguments(built):
    ctx = _ctx("box", 16, 16)
    seeds = orc.block_seeds(0, 16, 16)
    for strategy in ((0, -1), (0, 7), (1, -1), (1, 6), (2, 0), (-1, 0)):                                                        # (family, strategy)
        assert _code(ctx.render_point_normal_ats, seeds, strategy) == RL_ERR_INVALID_ARGUMENT, strategy
    for name in ("pn_best_ex", "eq_warp_ex"):
        with pytest.raises(ValueError):
            ctx.render_point_normal_ats(seeds, name)
    for kw, code in (({"spp": 0}, RL_ERR_INVALID_ARGUMENT), ({"shard_index": 2, "shard_count": 2}, RL_ERR_INVALID_ARGUMENT),
                     ({"stream_mode": api.STREAM_STRATIFIED}, api.RL_ERR_UNSUPPORTED), ({"stream_mode": 3}, RL_ERR_INVALID_ARGUMENT)):
        assert _code(ctx.render_point_normal_ats, seeds, "eq_ex", **kw) == code, kw
    assert _code(ctx.render_point_normal_ats, seeds[:0]) == RL_ERR_INVALID_ARGUMENT


def test_the_reach_of_the_jump_uses_the_trees_draw_count(built):
    """256 * spp * D <= 2^32 - 1 with D = 6 for eq_ex over the tree (the power pick's is 7): the largest spp that passes is refused one higher, and the
    restatement says the same; per-sample streams and the chain-pass strategies have no jump."""
    ctx = _ctx("box", 16, 16)
    seeds = orc.block_seeds(0, 16, 16)
    limit = 0xffffffff // (256 * 6)
    assert 256 * (limit + 1) * 6 > 0xffffffff >= 256 * limit * 6
    assert _code(ctx.render_point_normal_ats, seeds, "eq_ex", limit + 1) == api.RL_ERR_UNSUPPORTED
    with pytest.raises(A.Refused) as e:
        A.check_params("eq_ex", limit + 1, REF, 0, 1)
    assert e.value.code == api.RL_ERR_UNSUPPORTED
    A.check_params("eq_ex", limit, REF, 0, 1)
    A.check_params("eq_ex", limit + 1, REF, 0, 1, use_aa=False)                                 # D = 4 without the jitter
    A.check_params("pn_ex", limit + 1, REF, 0, 1)


# ---- mirrors
@pytest.mark.parametrize("strategy,use_aa,mode", [("eq_ex", True, REF), ("eq_clamped_ex", False, PER), ("eq_tr_taylor_ex", True, REF)])
def test_integrator_compute(built, strategy, use_aa, mode):
    sd = A.scene("lights8")
    integ = api.IntegratorPointNormalAts(strategy, use_aa, mode)
    img = integ.compute(api.IndependentSampler(9), api.Scene(sd), 2)
    ref = A.compute(sd, 9, strategy, 2, use_aa, mode)
    assert img.any() and img.tobytes() == ref["image"].tobytes()
    for k in P.COUNTERS:
        assert integ.last_stats[k] == ref["stats"][k], k


def test_the_cli_line_renders_what_the_binding_renders(built, tmp_path):
    """`data/cbox.pbrt -n 2 -s 0.0625 -m 1.0 -r independent:7 point-normal-ats -s pn_ex`, with and without `-x ats` in front: the image of
    IntegratorPointNormalAts on the same box at 32 x 32 (the C++ mirror against the Python one)."""
    scn = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "cbox.pbrt")
    sd = scenes.cbox_medium(32, 32, 1.0)
    sd.use_ats = True
    want = api.IntegratorPointNormalAts("pn_ex").compute(api.IndependentSampler(7), api.Scene(sd), 2)
    assert want.any()
    for front in ((), ("-x", "ats")):
        out = str(tmp_path / "pnats.pfm")
        r = subprocess.run([cli.EXE, scn, "-n", "2", "-s", "0.0625", "-m", "1.0", "-r", "independent:7", "-o", out, *front, "point-normal-ats", "-s", "pn_ex"],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        np.testing.assert_array_equal(api.load_pfm(out), np.abs(want))      # (save_pfm writes |value|)
