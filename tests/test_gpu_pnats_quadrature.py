"""The point-normal strategies over the light tree on the device held to tests/volume_quadrature.py, the float64 single-scattering quadrature that shares no
code with the kernel or the restatement, in the frame of tests/test_gpu_pn_quadrature.py, unchanged in method: 24 x 18, black walls, pixel-centre rays (AA
off), K = 8 seeds, volume_quadrature.check_ratios over r_k = mean(image_k) / mean(quadrature): SE(r) <= 5 % and |mean(r) - 1| <= 4 SE(r) + the quadrature's
error, at most 10 % of the pixels masked (asserted).

Scenes: `two`, the two-light scene of tests/test_gpu_pn_quadrature.py::test_two_lights with the tree (four proxies), and `lights8`, the eight quads of
tests/pnats_restatement.py with constant emission (the quadrature's RectLight has one colour per light; the HSV quad is held bit for bit in
tests/test_gpu_pnats_exact.py).  Cases: eq_ex, pn_ex, eq_clamped_ex, tr_ex and eq_tr_taylor_ex over the tree, and eq_ex on per-sample streams.
eq_clamped_phase stays out with several lights, for the reason tests/test_gpu_pn_quadrature.py gives.

The spp per case is found as that file finds it: the smallest power of two at which the restatement's spread of r over K = 8 seeds on the CPU
(scratch/pnats_spread.py) puts SE(r) under 2.5 %, i.e. a single-image spread under 0.0707.  profiles/pnats_note.md has the figures, and the restatement alone
passes this check on both scenes at these spp.  The ray importance is a bound with approximations: where it gives a light that does reach the ray
importance 0 the estimator is biased, as the reference's is; the placements here are ones for which the restatement's means show none."""
import pytest

from oracle import orc
from rustlight_amd import api
from tests import pn_restatement as P
from tests import pnats_restatement as A
from tests import test_gpu_pn_quadrature as PQ
from tests import volume_quadrature as Q
from tests.scene_helpers import black_walls, context as _context
from tests.test_gpu_pnmis_quadrature import ratios

pytestmark = pytest.mark.gpu

W, H, K, CAM_SEED = PQ.W, PQ.H, PQ.K, PQ.CAM_SEED
CASES = (("eq_ex", "two"), ("pn_ex", "two"), ("eq_clamped_ex", "two"), ("tr_ex", "two"), ("eq_tr_taylor_ex", "two"),
         ("eq_ex", "lights8"), ("pn_ex", "lights8"), ("eq_clamped_ex", "lights8"), ("tr_ex", "lights8"), ("eq_tr_taylor_ex", "lights8"))
SPP = {("eq_ex", "two"): 2, ("pn_ex", "two"): 2, ("eq_clamped_ex", "two"): 2, ("tr_ex", "two"): 4096, ("eq_tr_taylor_ex", "two"): 2,
       ("eq_ex", "lights8"): 8, ("pn_ex", "lights8"): 4, ("eq_clamped_ex", "lights8"): 4, ("tr_ex", "lights8"): 8192, ("eq_tr_taylor_ex", "lights8"): 8}


def scene(name, use_ats=True):
    sd = black_walls(A.scene({"two": "two_lights", "lights8": "lights8_const"}[name], W, H))
    sd.use_ats = use_ats
    return sd


class _Reference:
    """The quadrature through the pixel centres, per scene, computed once and left unchanged."""

    def __init__(self):
        self._centres = {}

    def centres(self, name):
        if name not in self._centres:
            sd = scene(name, use_ats=False)                                                  # the same geometry: the tree changes no radiance
            fr = P.Frame(sd)
            px, py, o, d, tfar = P.camera_rays(fr, orc.block_seeds(0, W, H), "tr_ex", 1, use_aa=False)
            keep = ~Q.near_a_light(sd, o, d, tfar, Q.NEAR)
            assert keep.mean() >= 0.9, "more than 10 % of the pixels masked"
            value, error = Q.image_mean(fr.sc, sd, o, d, tfar, keep)
            self._centres[name] = {"px": px, "py": py, "keep": keep, "value": value, "error": error}
        return self._centres[name]


@pytest.fixture(scope="module")
def reference(built):
    return _Reference()


def _check(reference, strategy, name, mode=api.STREAM_REFERENCE_ORDER):
    ref = reference.centres(name)
    ctx = _context(scene(name))
    spp = SPP[(strategy, name)]

    def render(seeds):
        img, st = ctx.render_point_normal_ats(seeds, strategy, spp, False, mode)
        assert st["camera_samples"] == W * H * spp
        return img

    return Q.check_ratios(f"point-normal-ats {strategy} {name}", ratios(ref, render), ref["error"] / ref["value"])


@pytest.mark.parametrize("strategy,name", CASES)
def test_every_case_reaches_the_quadrature(reference, strategy, name):
    """The pick's probability in the flux: a pdf_sel that is not the probability the walk picked the light with moves the mean, per channel where the
    lights differ in colour."""
    assert len(Q.lights_of(scene(name))) == {"two": 2, "lights8": 8}[name]
    _check(reference, strategy, name)


def test_per_sample_streams_reach_the_quadrature(reference):
    _check(reference, "eq_ex", "lights8", mode=api.STREAM_PER_SAMPLE)
