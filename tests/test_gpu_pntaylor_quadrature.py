"""The point-normal Taylor strategies on the device held to tests/volume_quadrature.py, the float64 single-scattering quadrature that shares no code with the
kernel or the restatement, in the frame of tests/test_gpu_pn_quadrature.py, whose scene and reference are imported: 24 x 18, the Cornell box with its medium
and black walls, AA off, K = 8 seeds, volume_quadrature.check_ratios over r_k = mean(image_k) / mean(quadrature) (at most 10 % of the pixels masked, asserted
by the reference): SE(r) <= 5 % and |mean(r) - 1| <= 4 SE(r) + the quadrature's error.

Media: `grey` (isotropic, sigma_s = 1) for the transmittance polynomials, `grey_hg` (the same with Henyey-Greenstein g = 0.6) for the phase polynomials —
in an isotropic medium the eq phase polynomials are the plain strategies and pn_phase_taylor_ex is refused —, and `two`, the grey medium with the second light.

The spp per case follows the rule of profiles/pn_note.md — the restatement's single-image spread of r on the CPU (scratch/pntaylor_spread.py, 8 seeds, AA off),
then the smallest power of two that puts SE(r) over K = 8 under 2.5 %, i.e. a single-image spread of 0.0707.  Measured at 8 spp the spread is 0.014 to 0.035
and the rule gives 1 or 2; measured at 2 spp it is 0.022 to 0.10 with the means one to two standard errors low, and the rule gives 1 to 8: the spread does not
follow 1 / sqrt(spp) from so few samples, so every case runs at the largest figure the rule gives, 8 spp, where the restatement's means over 8 seeds are 1.001
to 1.016, within two of their standard errors.  No strategy shows a bias in these media, so none is left out.  profiles/pntaylor_note.md has the table and what the
assertion catches on the CPU (pntaylor_restatement.MUTATION): the polynomial's pdf without its division by norm fails it; without its prob_poly factor, a
change of under 1 % in these scenes, it passes — that factor is held bit for bit and by the samplers' self-checks."""
import pytest

from oracle import orc  # noqa: F401  (scratch/pntaylor_spread.py takes it from here)
from rustlight_amd import api
from tests import pntaylor_restatement as T
from tests import test_gpu_pn_quadrature as PQ
from tests import volume_quadrature as Q
from tests.scene_helpers import context as _context
from tests.test_gpu_pn_quadrature import reference  # noqa: F401  (the module-scoped fixture: one quadrature per scene)
from tests.test_gpu_pnmis_quadrature import ratios

pytestmark = pytest.mark.gpu

W, H, K, CAM_SEED = PQ.W, PQ.H, PQ.K, PQ.CAM_SEED
PQ.MEDIA.setdefault("grey_hg", ((1.0,) * 3, (0.0,) * 3, 0.6))
TR = ("eq_tr_taylor_ex", "eq_clamped_tr_taylor_ex", "pn_tr_taylor_ex")
PHASE = ("eq_phase_taylor_ex", "eq_clamped_phase_taylor_ex", "pn_phase_taylor_ex")
CASES = tuple((s, "grey") for s in TR) + tuple((s, "grey_hg") for s in PHASE) + (("eq_tr_taylor_ex", "two"), ("pn_tr_taylor_ex", "two"))
SPP = {case: 8 for case in CASES}


def medium_of(medium):
    """(the name in MEDIA, second light)."""
    return ("grey", True) if medium == "two" else (medium, False)


def _check(reference, strategy, medium, mode=api.STREAM_REFERENCE_ORDER):  # noqa: F811
    name, two = medium_of(medium)
    ref = reference.centres(name, two)
    ctx = _context(PQ._scene(name, two))
    spp = SPP[(strategy, medium)]

    def render(seeds):
        img, st = ctx.render_point_normal_taylor(seeds, strategy, spp, False, mode)
        assert st["camera_samples"] == W * H * spp
        return img

    return Q.check_ratios(f"point-normal-taylor {strategy} {medium}", ratios(ref, render), ref["error"] / ref["value"])


@pytest.mark.parametrize("strategy,medium", CASES)
def test_every_strategy_reaches_the_quadrature(reference, strategy, medium):  # noqa: F811
    """The polynomial's normalisation, prob_poly, the inversion, the part beyond the clamp angle and the Jacobian: a pdf that does not integrate to one, or a
    sample that is not distributed by it, moves the mean."""
    if medium == "two":
        assert len(Q.lights_of(PQ._scene("grey", True))) == 2
    _check(reference, strategy, medium)


def test_per_sample_streams_reach_the_quadrature(reference):  # noqa: F811
    _check(reference, "eq_tr_taylor_ex", "grey", mode=api.STREAM_PER_SAMPLE)
