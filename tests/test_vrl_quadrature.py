"""tests/vrl_quadrature.py held to itself and to a closed form, and the setting of tests/test_gpu_vrl_quadrature.py checked without a GPU: the numpy
restatement (tests/vrl_restatement.py) alone meets the physics check there, and stops meeting it when one factor of the estimator is left out.

The setting.  The Cornell box with black walls and a medium of sigma_s = 0.7, sigma_a = 0.3, seen through a 6 degree lens, 24 x 18 pixels at 1 spp: the
frustum is a narrow shaft through the middle of the box and every ray ends on the back wall or a box (no ray misses, asserted: the estimator gives a missing
ray nothing, the pair integral to infinity is not nothing).  Two hand-made VRLs lie 0.4 and more beside the shaft — the estimator's 1 / r^2 has no finite
variance for a VRL the rays come arbitrarily near to, and the check needs SE <= 5 % —, a black surface beam stands for the beam tree, and black VRLs bring avg
down: 400 of them make rr = 1 for the two bright ones, 148 make rr = 0.75, the case that sees a missing 1 / rr.  K = 8 seeds, one ratio per seed and channel:
mean over the frame of the render / mean of the quadrature along the same rays; volume_quadrature.check_ratios asserts SE <= 5 % and |mean - 1| <= 4 SE + the
quadrature's error, the difference between the rules of order 32 and 16.  The figures are in profiles/vrl_note.md."""
import functools

import numpy as np
import pytest

from oracle import orc
from rustlight_amd import scenes
from tests import beam_restatement as R
from tests import volume_quadrature as VQ
from tests import vrl_quadrature as Q
from tests import vrl_restatement as V
from tests.scene_helpers import black_walls

W, H, K = 24, 18, 8
CAM_SEED = 2000
FOV = 6.0
SIGMA_S, SIGMA_A = (0.7,) * 3, (0.3,) * 3
N_PATHS, RADIUS, ORDER = 3, 0.1, 32
VRLS = [((0.45, 1.55, 0.7), (0.0, 0.0, -1.0), 0.8, (300.0, 200.0, 100.0)), ((-0.5, 0.45, 0.9), (0.6, 0.0, -0.8), 0.5, (100.0, 200.0, 300.0))]
N_BLACK = {"rr=1": 400, "rr=0.75": 148}
DROPS = {"sigma_s": "rr=1", "inv_pdf": "rr=1", "dist2": "rr=1", "rr": "rr=0.75"}      # the factor left out: the case that sees it


def scene():
    sd = black_walls(scenes.cbox(W, H, scenes.Medium(SIGMA_A, SIGMA_S, scenes.PHASE_ISOTROPIC, 0.0)))
    sd.fov = FOV
    return sd


def words_of(case):
    """A black surface beam (the map needs one), the two bright VRLs, then the black ones."""
    surface = R.beam_words([(0.0, 1.9, 0.0)], 0.3, [(0.0, -1.0, 0.0)], [(0.0, 0.0, 0.0)])
    bright = np.concatenate([R.beam_words([a], length, [b], [rad], from_surface=False) for a, b, length, rad in VRLS])
    black = R.beam_words(np.zeros((N_BLACK[case], 3)) + (0.0, 1.0, 0.0), 0.1, [(1.0, 0.0, 0.0)], [(0.0, 0.0, 0.0)], from_surface=False)
    return np.concatenate([surface, bright, black])


@functools.lru_cache(maxsize=None)
def reference():
    """[K] of {"seeds", "px", "py", "value" [3], "error" [3]}: the quadrature along each seed's camera rays, computed once."""
    sd = scene()
    sc = orc.Scene(sd)
    sigma_t = np.asarray(SIGMA_S) + np.asarray(SIGMA_A)
    out = []
    for k in range(K):
        seeds = orc.block_seeds(CAM_SEED + k, W, H)
        px, py, o, d, tfar, _, _, _ = V.camera_walk(sc, sd, seeds, 1, [])
        assert (tfar < V.F32_MAX).all(), "a camera ray misses the scene"
        value, error = Q.pair_integral_with_error(sc, VRLS, o, d, tfar, SIGMA_S, sigma_t, ORDER, N_PATHS)
        out.append({"seeds": seeds, "px": px, "py": py, "value": value.mean(axis=0), "error": error.mean(axis=0)})
    return out


def ratios(render, case):
    """[K, 3]: render(words, seeds) -> image, against the quadrature."""
    words = words_of(case)
    return [render(words, ref["seeds"])[ref["py"], ref["px"]].mean(axis=0) / ref["value"] for ref in reference()]


def quadrature_error():
    return np.max([ref["error"] / ref["value"] for ref in reference()], axis=0)


def _restatement(drop=None):
    sd = scene()
    sc = orc.Scene(sd)
    return lambda words, seeds: V.render(sc, sd, words, N_PATHS, seeds, 1, RADIUS, drop=drop)[0]


def test_the_cases_have_the_roulette_they_are_named_for(built):
    for case, want in (("rr=1", 1.0), ("rr=0.75", 0.75)):
        rr = V.roulette(V.partition(words_of(case))[1])[1]
        assert np.allclose(rr[:2], want, rtol=1e-6) and not rr[2:].any(), case


def test_order_doubling_converges(built):
    sd = scene()
    sc = orc.Scene(sd)
    _, _, o, d, tfar, _, _, _ = V.camera_walk(sc, sd, orc.block_seeds(CAM_SEED, W, H), 1, [])
    pick = slice(None, None, 37)
    sigma_t = np.asarray(SIGMA_S) + np.asarray(SIGMA_A)
    vals = [Q.pair_integral(sc, VRLS, o[pick], d[pick], tfar[pick], SIGMA_S, sigma_t, n, N_PATHS).mean(axis=0) for n in (8, 16, 32, 64)]
    steps = [np.abs(a - b).max() / vals[-1].max() for a, b in zip(vals, vals[1:])]
    print("relative steps 8->16->32->64:", steps)
    assert steps[1] <= 0.02 and steps[2] <= 0.01 and steps[2] <= steps[0]       # the rim of the box is a kink in V: algebraic, not spectral, convergence
    assert np.all(quadrature_error() <= 0.01)


def test_short_vrl_in_a_near_vacuum(built):
    """A VRL of length 0.01 at 0.6 from the ray, sigma_t = 1e-5: the rule against (theta_b - theta_a) / h * length.  The VRL's extent changes 1 / r^2 by
    (0.005 / 0.6)^2 < 1e-4 and the transmittance is above 1 - 1e-4: 1e-3 covers both and the rule's own error."""
    sd = scene()
    sc = orc.Scene(sd)
    o, d = sc.camera_generate(W / 2, H / 2)
    t, _, _, mesh, _ = sc.trace(o[None, :], d[None, :])
    assert mesh[0] >= 0
    vrl = ((0.0, 1.6, 0.5), (1.0, 0.0, 0.0), 0.01, (3.0, 2.0, 1.0))
    sigma = (1e-5,) * 3
    want = Q.short_vrl_closed_form(vrl, o, d, t[0], sigma, 2)
    got = Q.pair_integral(sc, [vrl], o[None, :], d[None, :], t[:1], sigma, sigma, 64, 2)[0]
    assert np.all(want > 0)
    np.testing.assert_allclose(got, want, rtol=1e-3)


def test_the_restatement_meets_the_physics_check(built):
    for case in N_BLACK:
        mean, se, _ = VQ.check_ratios(f"virtual-ray-lights restatement {case}", ratios(_restatement(), case), quadrature_error())
        assert np.all(se <= 0.05)


@pytest.mark.parametrize("drop", sorted(DROPS))
def test_a_missing_factor_breaks_it(built, drop):
    case = DROPS[drop]
    rs = ratios(_restatement(drop), case)
    mean, se = VQ.ratio_statistic(rs)
    print(f"without {drop} ({case}): r = {mean} +- {se}")
    with pytest.raises(AssertionError):
        VQ.check_ratios(f"virtual-ray-lights restatement without {drop}", rs, quadrature_error())
