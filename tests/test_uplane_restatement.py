"""tests/uplane_restatement.py held on the CPU before anything on the device is compared with it: its numpy xoshiro256++ against orc.Rng; the draw count
samples * D + 2 * redraws against a literal walk that counts its draws; the literal scalar walk of one small block (plane_single_restatement's own pieces,
plane after plane) against the form over arrays, in every strategy and through a redraw; every image fixture of tests/test_gpu_uplane_exact.py non-zero in
at least a quarter of its pixels; each redraw case reporting its redraw at the stated lane, sample and plane with a lit pixel on a later lane of that block."""
import numpy as np
import pytest

from oracle import orc
from rustlight_amd import scenes
from tests import uplane_restatement as U
from tests.scene_helpers import two_lights


def test_numpy_xoshiro_is_the_oracles(built):
    for seed, variant in ((0, 0), (303, 0), (2 ** 63 + 5, 1)):
        rng = orc.Rng(seed, variant)
        want = np.asarray([rng.next_f32() for _ in range(3 * U._SUB + 7)], np.float32)
        np.testing.assert_array_equal(U.stream(seed, variant, want.shape[0]), want)
        np.testing.assert_array_equal(U.draws_at(seed, variant, 2 * U._SUB + 3, 4), want[2 * U._SUB + 3:2 * U._SUB + 7])


def test_the_zeros_the_redraw_cases_stand_on(built):
    """Rng(303, 0) draws exactly 0.0 at index 91307 between 0.60031056 and 0.10098672, Rng(196, 0) at 226623 between 0.48445052 and 0.6417996, and neither
    draws another zero among its first 300 000; both zeros give z == 0 as a first and as a second coordinate."""
    for seed, at, before, after in ((303, 91307, 0.60031056, 0.10098672), (196, 226623, 0.48445052, 0.6417996)):
        s = U.stream(seed, 0, 300000)
        np.testing.assert_array_equal(np.flatnonzero(s == 0.0), [at])
        np.testing.assert_array_equal(U.zero_draws(seed, 0, 300000), [at])
        assert s[at - 1] == np.float32(before) and s[at + 1] == np.float32(after)
        assert U._hemisphere(s[at:at + 1], s[at + 1:at + 2])[0, 2] == 0.0 and U._hemisphere(s[at - 1:at], s[at:at + 1])[0, 2] == 0.0
        assert U.R.cosine_sample_hemisphere(s[at], s[at + 1])[2] == 0.0 and U.R.cosine_sample_hemisphere(s[at - 1], s[at])[2] == 0.0


def _same_block(a, b):
    np.testing.assert_array_equal(a["rgb"], b["rgb"])
    np.testing.assert_array_equal(a["px"], b["px"])
    np.testing.assert_array_equal(a["py"], b["py"])
    for k in ("samples", "redraws", "draws", "intersected", "visible"):
        assert a[k] == b[k], k


@pytest.mark.parametrize("strategy", U.STRATEGIES)
def test_scalar_walk_equals_the_array_form(built, strategy):
    """A 5 x 3 frame (one ragged block), 2 spp, in a medium with a sigma_t per channel; then the box with two lights.  24 planes, more where a plane meets a
    ray too seldom for 24 to meet any (uv, vt)."""
    nb = {"uv": 256, "vt": 128}.get(strategy, 24)
    for sd in (scenes.cbox(5, 3, scenes.Medium((0.2, 0.1, 0.0), (0.5, 0.9, 1.4), scenes.PHASE_ISOTROPIC, 0.0)), two_lights(5, 3)):
        sc = orc.Scene(sd)
        a = U.render_block(sc, sd, U._Lights(U.R.rect_lights(sd)), 0, 7, nb, strategy, 2)
        b = U.walk_block(sc, sd, 0, 7, nb, strategy, 2)
        _same_block(a, b)
        assert a["draws"] == a["samples"] * U.draws_per_sample(nb, strategy) and a["visible"] > 0


def test_scalar_walk_equals_the_array_form_through_a_redraw(built):
    """Rng(303, 0) on a 4 x 2 frame at 2 spp and 951 planes under average: its zero is the second coordinate of plane 949 of lane 5's second sample.  The walk
    counts its draws one by one: samples * D + 2 * redraws."""
    sd = scenes.cbox_medium(4, 2, 1.0)
    sc = orc.Scene(sd)
    a = U.render_block(sc, sd, U._Lights(U.R.rect_lights(sd)), 0, 303, 951, "average", 2)
    b = U.walk_block(sc, sd, 0, 303, 951, "average", 2)
    _same_block(a, b)
    assert b["redraws"] == [(5, 1, 949)]
    assert b["draws"] == 16 * U.draws_per_sample(951, "average") + 2
    zeros = U.zero_draws(303, 0, b["draws"])
    s = U.stream(303, 0, b["draws"] + 8)
    assert U.zero_redraws(zeros, lambda i: (s[i], s[i + 1]), 951, "average") == [(11, 949)]


@pytest.mark.parametrize("strategy", U.STRATEGIES)
def test_fixture_is_lit_in_a_quarter_of_its_pixels(built, strategy):
    sd, seeds, nb, spp, img, st, detail = U.fixture(strategy)
    assert np.count_nonzero(img.any(axis=-1)) >= 0.25 * sd.width * sd.height
    assert st["camera_samples"] == sd.width * sd.height * spp and st["redraws"] == 0 and detail["corners_finite"]
    assert st["rng_draws"] == st["camera_samples"] * U.draws_per_sample(nb, strategy)
    assert st["planes_intersected"] >= st["planes_visible"] > 0


@pytest.mark.parametrize("i", range(len(U.REDRAW_CASES)))
def test_redraw_case_redraws_where_it_says(built, i):
    sd, seeds, block, (seed, strategy, nb, spp, lane, sample, plane), img, st, detail = U.redraw_case(i)
    assert detail["redraw_lanes"] == {block: [(lane, sample, plane)]}
    assert st["redraws"] == 1 and st["rng_draws"] == st["camera_samples"] * U.draws_per_sample(nb, strategy) + 2
    later = detail["blocks"][block]["rgb"][lane + 1:]
    assert later.any(), "no later lane of the block is lit"
    s = U.stream(seed, 0, detail["blocks"][block]["draws"] + 8)
    assert U.zero_redraws(np.flatnonzero(s == 0.0), lambda k: (s[k], s[k + 1]), nb, strategy) == [(lane * spp + sample, plane)]
