"""The point-normal strategies on the device held to tests/volume_quadrature.py, the float64 single-scattering quadrature that shares no code with the kernel
or the restatement, in the frame of tests/test_gpu_uplane_quadrature.py: 24 x 18 (2 x 2 blocks, both edges ragged), the Cornell box with its medium and black
walls, K = 8 seeds, volume_quadrature.check_ratios over r_k = mean(image_k) / mean(quadrature) along the integrator's own camera rays (at most 10 % of the
pixels masked, asserted): SE(r) <= 5 % and |mean(r) - 1| <= 4 SE(r) + the quadrature's error.

The rays.  With AA off every sample of a pixel looks through the pixel's centre, whatever the seed, the strategy and the spp: one quadrature per scene serves
every case, which is what lets tr_phase take the 32768 spp it needs.  One case (eq_ex, 4 spp) runs with AA on along its own jittered rays, found by
tests/pn_restatement.camera_rays from the block streams.

The spp per strategy is the smallest power of two that puts SE(r) over K = 8 under 2.5 %, half the bound, from the restatement's single-image spread on the
CPU with AA off (profiles/pn_note.md has the figures), the larger of the two media where both are rendered: tr_ex 0.21 (grey) and 0.31 (coloured) at 256 spp
over 16 seeds -> 4096 and 8192 (8192 is kept, one power of two above the grey medium's: the spread is known not to follow 1 / sqrt(spp); the
coloured case itself is left out, see its test); eq_ex 0.030 at 16 -> 4; eq_clamped_ex 0.037 at 4 -> 2; pn_ex 0.031 (grey) and 0.084 (coloured) at 4 -> 1 and 8; eq_phase 0.13
at 256 over 6 seeds -> 1024; eq_clamped_phase 0.19 at 32 -> 256; tr_phase 0.28 at 1024 -> 32768.  tr_ex has a heavy tail (the geometry term of a free path
that ends near the light): its spread fell from 0.36 at 16 spp to 0.21 at 256, slower than 1 / sqrt(spp), so a first estimate from 16 spp (512) was too low.

eq_clamped_phase is checked on the single-light scene only: with several lights the reference's estimator is biased (examples/cli.rs:466 says so) — the
clamp follows the light that was chosen, but the phase ray's hit on any light counts."""
import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import pn_restatement as P
from tests import volume_quadrature as Q
from tests.scene_helpers import add_second_light, black_walls, context as _context

pytestmark = pytest.mark.gpu

W, H, K = 24, 18, 8
CAM_SEED = 4000                                      # seed k renders with the block seeds of CAM_SEED + k
SPP = {"tr_ex": 8192, "tr_phase": 32768, "eq_ex": 4, "eq_phase": 1024, "eq_clamped_ex": 2, "eq_clamped_phase": 256, "pn_ex": 8}
MEDIA = {                                            # name: (sigma_s, sigma_a, g)
    "grey": ((1.0,) * 3, (0.0,) * 3, None),
    "coloured": (P.COLOURED[0], P.COLOURED[1], 0.6),
}


def _scene(medium, second_light=False):
    ss, sa, g = MEDIA[medium]
    sd = scenes.cbox(W, H, scenes.Medium(sa, ss, scenes.PHASE_ISOTROPIC if g is None else scenes.PHASE_HG, 0.0 if g is None else g))
    if second_light:
        add_second_light(sd)
    return black_walls(sd)


class _Reference:
    """The quadrature through the pixel centres, per scene, computed once and left unchanged."""

    def __init__(self):
        self._centres = {}

    def centres(self, medium, second_light):
        key = (medium, second_light)
        if key not in self._centres:
            sd = _scene(medium, second_light)
            fr = P.Frame(sd)
            px, py, o, d, tfar = P.camera_rays(fr, orc.block_seeds(0, W, H), "tr_ex", 1, use_aa=False)
            keep = ~Q.near_a_light(sd, o, d, tfar, Q.NEAR)
            assert keep.mean() >= 0.9, "more than 10 % of the pixels masked"
            value, error = Q.image_mean(fr.sc, sd, o, d, tfar, keep)
            self._centres[key] = {"px": px, "py": py, "keep": keep, "value": value, "error": error}
        return self._centres[key]


@pytest.fixture(scope="module")
def reference(built):
    return _Reference()


def _check(label, reference, strategy, medium="grey", second_light=False, mode=api.STREAM_REFERENCE_ORDER):
    ref = reference.centres(medium, second_light)
    ctx = _context(_scene(medium, second_light))
    rs = []
    for k in range(K):
        img, st = ctx.render_point_normal(orc.block_seeds(CAM_SEED + k, W, H), strategy, SPP[strategy], False, mode)
        assert st["camera_samples"] == W * H * SPP[strategy]
        rs.append(img[ref["py"], ref["px"]][ref["keep"]].mean(axis=0) / ref["value"])
    return Q.check_ratios(label, rs, ref["error"] / ref["value"])


@pytest.mark.parametrize("strategy", P.STRATEGIES)
def test_every_strategy_in_the_grey_medium(reference, strategy):
    """Isotropic, sigma_s = 1, one light: the distance pdfs, correct_flux, the geometry term, both transmittances."""
    _check(f"point-normal {strategy} grey", reference, strategy)


def test_per_sample_streams_reach_the_quadrature(reference, strategy="eq_ex"):
    _check(f"point-normal {strategy} grey, per-sample streams", reference, strategy, mode=api.STREAM_PER_SAMPLE)


@pytest.mark.parametrize("strategy", ["eq_ex", "pn_ex"])
def test_the_coloured_medium_with_a_forward_phase_function(reference, strategy):
    """sigma_s = (0.4, 1.0, 1.5) with sigma_a = (1.2, 0.6, 0.1) and Henyey-Greenstein g = 0.6: sigma_s where sigma_t belongs, or a phase function evaluated
    with a turned direction, is off by a different factor in every channel.  tr_ex is not among them: in this medium the restatement's spread on the CPU is
    still 0.30 at 4096 spp and 0.098 at 32768 (8 seeds; the geometry term's heavy tail), so SE(r) <= 2.5 % asks for 65536 spp or more on 432 lanes, seconds
    per image; the strategy is held to the quadrature in the grey medium and to the restatement, bit for bit, in this one (tests/test_gpu_pn_exact.py)."""
    _check(f"point-normal {strategy} coloured", reference, strategy, medium="coloured")


@pytest.mark.parametrize("strategy", ["eq_ex", "eq_clamped_ex", "pn_ex"])
def test_two_lights(reference, strategy):
    """The emitter pick and its pdf: the second light emits (4, 6, 9) where the first emits (17, 12, 4), so a wrong share shows per channel."""
    sd = _scene("grey", second_light=True)
    assert len(Q.lights_of(sd)) == 2
    _check(f"point-normal {strategy} two lights", reference, strategy, second_light=True)


def test_jittered_rays(built, strategy="eq_ex"):
    """AA on: the quadrature along the very camera rays of every seed, 4 per pixel."""
    sd = _scene("grey")
    fr = P.Frame(sd)
    ctx = _context(sd)
    spp = SPP[strategy]
    rs, errs = [], []
    for k in range(K):
        seeds = orc.block_seeds(CAM_SEED + k, W, H)
        px, py, o, d, tfar = P.camera_rays(fr, seeds, strategy, spp)
        near = Q.near_a_light(sd, o, d, tfar, Q.NEAR)
        bad = np.zeros((H, W), bool)
        bad[py[near], px[near]] = True                                  # a pixel is left out with all its samples
        assert bad.mean() <= 0.1, "more than 10 % of the pixels masked"
        value, error = Q.image_mean(fr.sc, sd, o, d, tfar, ~bad[py, px])
        img, st = ctx.render_point_normal(seeds, strategy, spp)
        rs.append(img[~bad].mean(axis=0) / value)
        errs.append(error / value)
    Q.check_ratios(f"point-normal {strategy} grey, jittered rays", rs, np.max(errs, axis=0))
