"""tests/pntaylor_restatement.py against itself and against closed forms (no GPU): the scalar walk equals the vectorised render, bit for bit, for the six
strategies; the codes of check_params and of the medium's refusal; the two eq phase polynomials in an isotropic medium are the plain strategies' bytes; the
samplers' self-checks in float64 — the returned pdf is the sampler's density, the density integrates to one over the range, and the integral up to sample(u)
gives u back — at geometries where the polynomial is positive over the range; both outcomes of every `new`'s None test and both branches of sample() met and
counted; Poly6 against its closed forms; the Newton / bisection solver on a cubic."""
import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import pn_restatement as P
from tests import pntaylor_restatement as T

F32 = np.float32
MODES = (api.STREAM_REFERENCE_ORDER, api.STREAM_PER_SAMPLE)
TR = ("eq_tr_taylor_ex", "eq_clamped_tr_taylor_ex", "pn_tr_taylor_ex")
# Newton stops at |pos| * 2^-9 >= |delta| (math.rs:219): the last step it takes is below |pos| / 512, and with a quadratically converging step the
# position it returns is much closer than that.  Over the 4 geometries x 199 values of u below the restatement shows, between the integral of its density
# over the range and 1, at most 6.2e-7, and between the integral up to sample(u) and u at most 2.7e-6 — float32 in the normalisation, not the solver's stop;
# pn_phase_taylor_ex shows 2.7e-5 and 7.9e-5: cdf_pn's coefficients reach 360 t6 = 103 for g = 0.6 and cancel in float32.  The bounds are twice these
# figures (profiles/pntaylor_note.md).  {strategy is pn_phase_taylor_ex: (density integral, integral up to the sample)}
TOLERANCES = {False: (1.3e-6, 5.4e-6), True: (5.4e-5, 1.6e-4)}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("strategy", T.STRATEGIES)
def test_scalar_walk_equals_vectorised_render_in_the_coloured_medium(strategy, mode):
    fr = T.frame("coloured")
    seeds = orc.block_seeds(11, 24, 18)
    a = T.render(fr, seeds, strategy, 2, True, mode)
    b = T.render_walk(fr, seeds, strategy, 2, True, mode)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and a[1] == b[1]
    assert all(a[2][k] == b[2][k] for k in ("some", "none") + T.EXTRA)
    if mode == api.STREAM_REFERENCE_ORDER:
        assert all(np.array_equal(a[2]["starts"][k], b[2]["starts"][k]) for k in a[2]["starts"])
    assert a[0].any() and a[2]["took_poly"] > 0 and a[2]["newton_steps"] > 0


@pytest.mark.parametrize("use_aa", (True, False))
@pytest.mark.parametrize("strategy", TR)
@pytest.mark.parametrize("name", ("lights", "floating"))
def test_scalar_walk_equals_vectorised_render_where_samplers_are_none(name, strategy, use_aa):
    fr = T.frame(name)
    seeds = orc.block_seeds(11, 24, 18)
    a = T.render(fr, seeds, strategy, 2, use_aa)
    b = T.render_walk(fr, seeds, strategy, 2, use_aa)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and a[1] == b[1]
    assert all(a[2][k] == b[2][k] for k in ("some", "none") + T.EXTRA)
    assert all(np.array_equal(a[2]["starts"][k], b[2]["starts"][k]) for k in a[2]["starts"])
    st, det = a[1], a[2]
    assert det["some"] + det["none"] == st["camera_samples"] and st["vertices"] == det["some"]
    assert st["rng_draws"] == st["camera_samples"] * (6 if use_aa else 4) + det["some"] and st["extension_rays"] == st["camera_samples"]


def test_every_outcome_of_the_none_tests_and_both_branches_are_met():
    """Over the shared fixtures: new_clamping's None, PointNormalSampling::new's, the three arms of either Taylor `new`, sample < prob_poly and its else."""
    total = {k: 0 for k in ("some", "none") + T.EXTRA}
    for name, strategies in (("coloured", T.STRATEGIES), ("floating", TR), ("lights", TR)):
        for s in strategies:
            det = T.fixture(name, s)[4]
            assert det["none"] == det["none_base"] + det["none_pn"] + det["none_poly"]
            assert det["some"] == det["branch_low"] + det["branch_mixed"] + det["branch_all"] == det["took_poly"] + det["took_other"]
            for k in total:
                total[k] += det[k]
    for k in ("some", "none_base", "none_pn", "branch_low", "branch_mixed", "branch_all", "took_poly", "took_other", "newton_steps"):
        assert total[k] > 0, k
    det = T.fixture("floating", "pn_tr_taylor_ex")[4]
    assert det["none_pn"] > 0 and det["none_base"] > 0 and det["branch_low"] > 0 and det["took_other"] > 0 and det["took_poly"] > 0
    det = T.fixture("floating", "eq_clamped_tr_taylor_ex")[4]
    assert det["branch_low"] > 0 and det["branch_mixed"] > 0 and det["took_other"] > 0


# ---- one camera ray and one light point, by hand: o = 0, d = +z, max_dist = 2.5
O = np.zeros((1, 3), F32)
D = np.asarray([[0.0, 0.0, 1.0]], F32)
MAX = np.asarray([2.5], F32)
GEOMETRIES = {   # name: (light position, normal)
    "clamped before the clamp angle": ((0.7, 0.0, 0.4), (-0.6, 0.0, -0.8)),      # the light's plane cuts the ray at 0.925: theta_b = 0.64, the polynomial alone
    "side light": ((0.7, 0.0, 0.4), (-1.0, 0.0, 0.0)),                           # d . n = 0: no clamp, theta_b = 1.25 passes the clamp angle — both parts
    "far side light": ((1.5, 0.0, 1.0), (-1.0, 0.0, 0.0)),
    "near light": ((0.3, 0.0, 0.2), (-1.0, 0.0, 0.0)),
}


def _medium():
    return T.frame("coloured").medium                   # sigma_t = 1.6 in every channel, Henyey-Greenstein g = 0.6


def _sampler(strategy, geometry):
    pos, nrm = GEOMETRIES[geometry]
    s, ok, why = T.make_sampler(strategy, _medium(), np.asarray([True]), MAX, O, D, np.asarray([pos], F32), np.asarray([nrm], F32))
    assert ok[0], (strategy, geometry)
    return s


def _density_integral(strategy, s, upto, n=40001):
    """The integral of the sampler's angular density from theta_a to each of `upto`, float64 midpoints; the clamp angle is made an edge of the grid."""
    ta, clamp = float(s["theta_a"][0]), float(s["clamp"][0])
    out = []
    for hi in np.atleast_1d(upto):
        total = 0.0
        for lo_, hi_ in ((ta, min(hi, clamp)), (clamp, hi)):
            if hi_ > lo_:
                edges = np.linspace(lo_, hi_, n)
                mid = 0.5 * (edges[1:] + edges[:-1])
                total += float(np.sum(T.sampler_pdf(strategy, s, mid) * np.diff(edges)))
        out.append(total)
    return np.asarray(out)


@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("strategy", T.STRATEGIES)
def test_sampler_self_checks(strategy, geometry):
    s = _sampler(strategy, geometry)
    ta, tb, clamp = float(s["theta_a"][0]), float(s["theta_b"][0]), float(s["clamp"][0])
    # the polynomial is positive over the part of the range it covers, so the density is one
    grid = np.linspace(ta, min(tb, clamp), 2001)
    assert (sum(float(s["t"][i][0]) * grid ** i for i in range(7)) > 0).all(), "choose a geometry whose polynomial is positive over the range"
    one = _density_integral(strategy, s, [tb])[0]
    print(f"{strategy} {geometry}: integral of the density {one:.9f}")
    u = np.linspace(0.005, 0.995, 199).astype(F32)
    rep = {k: ([np.repeat(c, u.shape[0]) for c in v] if k == "t" else np.repeat(v, u.shape[0])) for k, v in s.items()}
    t, pdf, flags = T.sample_taylor(strategy, rep, u)
    assert not flags["div_zero"].any()
    if float(s["prob"][0]) < 1.0:
        assert flags["took_poly"].any() and flags["took_other"].any()
    theta = np.arctan((t.astype(np.float64) - float(s["delta"][0])) / float(s["d_l"][0]))
    assert (theta >= ta - 1e-6).all() and (theta <= tb + 1e-6).all()
    # the returned pdf is the density at the sampled angle times the Jacobian d_l / (d_l^2 + t^2): float32 through tan and the polynomial
    d_l = float(s["d_l"][0])
    jac = d_l / (d_l ** 2 + (t.astype(np.float64) - float(s["delta"][0])) ** 2)
    np.testing.assert_allclose(pdf, T.sampler_pdf(strategy, s, theta) * jac, rtol=2e-4)
    # the integral of the density up to the sampled angle gives the draw back
    cdf = _density_integral(strategy, s, theta, n=4001)
    err = float(np.max(np.abs(cdf - u.astype(np.float64))))
    print(f"{strategy} {geometry}: |integral up to sample(u) - u| <= {err:.3e}, Newton steps mean {flags['newton_steps'][flags['took_poly']].mean():.2f} "
          f"max {int(flags['newton_steps'].max())}")
    tol_one, tol_cdf = TOLERANCES[strategy == "pn_phase_taylor_ex"]
    assert abs(one - 1.0) <= tol_one and err <= tol_cdf


def test_a_normalisation_that_is_not_positive_gives_none():
    """TaylorSampling::new's `norm <= 0` and PointNormalTaylorSampling::new's `norm_poly <= 0`: a camera ray that ends 2e-8 to 8e-6 from its origin, the light
    beside and behind it.  theta_a < theta_b holds from the first distance on, but the two angles are so close that the polynomial's cdf, or cdf_pn, over
    them rounds to zero or below: None for some of these rays, Some for the others, for every strategy."""
    med = _medium()
    max_dist = (np.arange(1, 400) * 2e-8).astype(F32)
    n = max_dist.shape[0]
    pos, nrm = np.repeat(np.asarray([[0.7, 0.0, -0.2]], F32), n, 0), np.repeat(np.asarray([[-1.0, 0.0, 0.0]], F32), n, 0)
    for strategy in T.STRATEGIES:
        s, ok, why = T.make_sampler(strategy, med, np.ones(n, bool), max_dist, np.repeat(O, n, 0), np.repeat(D, n, 0), pos, nrm)
        assert not why["none_base"].any() and not why["none_pn"].any() and (s["theta_a"] < s["theta_b"]).all()
        assert why["none_poly"].any() and ok.any() and (ok == ~why["none_poly"]).all() and why["branch_all"][ok].all(), strategy
        assert (s["norm"][why["none_poly"]] <= 0).all() and (s["norm"][ok] > 0).all()


def test_poly6_against_closed_forms():
    """phase(g) is the Taylor polynomial of (1 + g^2 + 2 g sin(theta))^(-3/2) and tr(x) that of exp(-x (tan(theta) + 1 / cos(theta) - 1)) about 0: near 0 the
    polynomial is the function to the seventh order; cdf is the polynomial's integral; cdf_pn is the integral of the polynomial times a cos + b sin."""
    theta = np.linspace(-0.2, 0.2, 9)
    for g in (0.6, -0.3, 0.0):
        t = [float(c) for c in T.poly_phase(g)]
        exact = (1.0 + g * g + 2.0 * g * np.sin(theta)) ** -1.5
        np.testing.assert_allclose(sum(t[i] * theta ** i for i in range(7)), exact, rtol=5e-5)
    x = np.asarray([1.12], F32)
    t = [float(c[0]) for c in T.poly_tr(x, F32(1.0))]
    exact = np.exp(-1.12 * (np.tan(theta) + 1.0 / np.cos(theta) - 1.0))
    np.testing.assert_allclose(sum(t[i] * theta ** i for i in range(7)), exact, rtol=5e-5)
    tf = [np.asarray([c], F32) for c in t]
    hi = np.asarray([0.7], F32)
    edges = np.linspace(-0.5, 0.7, 200001)
    mid = 0.5 * (edges[1:] + edges[:-1])
    p = sum(t[i] * mid ** i for i in range(7))
    assert abs(float(T.poly_cdf(tf, hi)[0] - T.poly_cdf(tf, np.asarray([-0.5], F32))[0]) - float(np.sum(p * np.diff(edges)))) < 1e-6
    a, b = np.asarray([0.8], F32), np.asarray([-0.3], F32)
    got = float(T.CdfPn(tf, a, b, np.asarray([-0.5], F32)).at(hi)[0])
    assert abs(got - float(np.sum(p * (0.8 * np.cos(mid) - 0.3 * np.sin(mid)) * np.diff(edges)))) < 2e-5      # coefficients of up to 360 t6 in float32
    assert float(T.clamp_angle_phase(0.6)) == pytest.approx(0.8975, abs=1e-3) and float(T.clamp_angle_tr(F32(1.6), np.asarray([0.7], F32))[0]) == pytest.approx(
        np.exp(0.210824 - 0.15974 * 0.7 * 1.6), rel=1e-6)
    assert float(T.powi(F32(1.5), 7)) == float(F32(1.5) ** 7) and float(T.powi(F32(3.0), 1)) == 3.0


def test_newton_on_a_cubic():
    """f(x) = x^3 on [0, 2] for y in (0, 8): at most 30 rounds, the stop of math.rs:219 — the last step is below |pos| / 512, the position much closer."""
    y = np.linspace(0.01, 7.9, 80).astype(F32)
    n = y.shape[0]

    def f_both(v, idx):
        return (v * v * v).astype(F32), (F32(3.0) * v * v).astype(F32)

    pos, div_zero, iters = T.newton(np.full(n, 1.0, F32), np.zeros(n, F32), np.full(n, 2.0, F32), y, f_both)
    assert not div_zero.any() and iters.max() <= 30 and iters.min() >= 1
    np.testing.assert_allclose(pos, np.cbrt(y.astype(np.float64)), rtol=2.0 ** -9)
    # a zero derivative where the function is not y: div_zero, and the position stays
    pos, div_zero, iters = T.newton(np.zeros(1, F32), np.full(1, -1.0, F32), np.ones(1, F32), np.full(1, 0.5, F32), f_both)
    assert div_zero[0] and pos[0] == 0.0 and iters[0] == 0


def test_refusals_carry_their_codes():
    for strategy, spp, mode, code in (("eq_tr_taylor_ex", 0, api.STREAM_REFERENCE_ORDER, P.RL_ERR_INVALID_ARGUMENT),
                                      ("eq_ex", 1, api.STREAM_REFERENCE_ORDER, P.RL_ERR_INVALID_ARGUMENT), ("pn_best_ex", 1, api.STREAM_REFERENCE_ORDER, P.RL_ERR_INVALID_ARGUMENT),
                                      ("eq_tr_taylor_ex", 1, api.STREAM_STRATIFIED, P.RL_ERR_UNSUPPORTED), ("eq_tr_taylor_ex", 1, 3, P.RL_ERR_INVALID_ARGUMENT)):
        with pytest.raises(T.Refused) as e:
            T.check_params(strategy, spp, mode, 0, 1)
        assert e.value.code == code, (strategy, spp)
    with pytest.raises(T.Refused) as e:
        T.check_params("eq_tr_taylor_ex", 1, api.STREAM_REFERENCE_ORDER, 2, 2)
    assert e.value.code == P.RL_ERR_INVALID_ARGUMENT
    T.check_params("pn_tr_taylor_ex", 1 << 21, api.STREAM_REFERENCE_ORDER, 0, 1)           # every strategy takes the chain pass: no jump, no reach
    assert all(T.draws_per_sample(s) is None for s in T.STRATEGIES)


def test_the_isotropic_medium_forwards_and_refuses():
    fr = T.frame("box")
    seeds = orc.block_seeds(5, 24, 18)
    for strategy, plain in (("eq_phase_taylor_ex", "eq_ex"), ("eq_clamped_phase_taylor_ex", "eq_clamped_ex")):
        assert T.forwarded(fr.medium, strategy) == plain and T.forwarded(T.frame("coloured").medium, strategy) is None
        for mode in MODES:
            a, b = T.render(fr, seeds, strategy, 2, True, mode), P.render(fr, seeds, plain, 2, True, mode)
            assert a[0].any() and np.array_equal(_bits(a[0]), _bits(b[0])) and a[1] == b[1]
    assert all(T.forwarded(fr.medium, s) is None for s in TR + ("pn_phase_taylor_ex",))
    for render in (T.render, T.render_walk):
        with pytest.raises(T.Refused) as e:
            render(fr, seeds, "pn_phase_taylor_ex", 1)
        assert e.value.code == P.RL_ERR_UNSUPPORTED
    # Henyey-Greenstein with g = 0 is g = 0 as well; the eq phase polynomials are built there (the reference matches on the phase function, not on g)
    med = P.Medium(scenes.Medium((0.0,) * 3, (1.0,) * 3, scenes.PHASE_HG, 0.0))
    with pytest.raises(T.Refused):
        T.check_medium(med, "pn_phase_taylor_ex")
    assert T.forwarded(med, "eq_phase_taylor_ex") is None
    T.check_medium(T.frame("coloured").medium, "pn_phase_taylor_ex")
