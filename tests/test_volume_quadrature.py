"""tests/volume_quadrature.py held to closed forms it shares no code with, its convergence on the scenes the tests use, and then the CPU yardsticks of the
volume integrators (the numpy restatements of plane-single and the beam radiance estimate, the oracle's path tracer) held to it at sizes the CPU affords.

The statistic (volume_quadrature.check_ratios): over K seeds of generation and camera, r_k = mean(image_k) / mean(quadrature on seed k's rays) per channel,
over the pixels whose ray does not come within NEAR of a light (a function of the rays alone; at most 10 % of the pixels, asserted).  Asserted:
SE(r) <= 5 % and |mean(r) - 1| <= 4 SE(r) + the quadrature's own error estimate.  The same statistic at the device's counts is
tests/test_gpu_volume_quadrature.py; the figures of both are in profiles/volume_quadrature_note.md."""
import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import bre_restatement as B
from tests import plane_single_restatement as P
from tests import volume_quadrature as Q
from tests.scene_helpers import black_walls, two_lights

NEAR = Q.NEAR             # rays closer than this to a light's quad are left out (the 3 x 3 .. 6 x 6 grid on a 0.47 x 0.38 light does not resolve them)
W, H = 12, 9


# ---- closed forms
def _lone_light(half_u, half_v, height, emission=(3.0, 2.0, 1.0), medium=None):
    """Nothing but a quad at y = height, centred on the y axis, emitting downwards: an unoccluded scene."""
    quad = [-half_u, height, -half_v, half_u, height, -half_v, half_u, height, half_v, -half_u, height, half_v]
    light = scenes._quad_mesh("light", quad, [0, -1, 0], scenes.matte((0, 0, 0)), emission=emission)
    to_world = np.asarray([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, -5, 1], dtype=np.float32)
    return scenes.SceneData(8, 8, 40.0, 0, to_world, False, [light], medium or scenes.Medium((0.0,) * 3, (1.0,) * 3))


def _both(sc, sd, o, d, tfar, media):
    """(value, error estimate) of one ray, [3] each, for the one medium of `media`."""
    v, e = Q.image_mean(sc, sd, np.asarray([o]), np.asarray([d]), np.asarray([tfar]), media=[media])
    return v[0], e[0]


def test_point_like_light_matches_the_closed_form(built):
    """A 0.004 x 0.004 quad 2 above the x axis, a ray along that axis passing 0.5 beside the point below the light, sigma_t -> 0, isotropic: the point-light
    in-scattering integral with a Lambertian emitter's cosine, int h / (s^2 + rho^2)^(3/2) ds = h / rho^2 [s / sqrt(s^2 + rho^2)] (rho^2 = h^2 + z0^2),
    times sigma_s Le A / (4 pi).  The quad's finite size changes it by O((size / rho)^2) < 4e-6, allowed on top of the error estimate."""
    e, h, z0 = 0.002, 2.0, 0.5
    sd = _lone_light(e, e, h)
    sc = orc.Scene(sd)
    rho2 = h * h + z0 * z0
    primitive = lambda s: h / rho2 * s / np.sqrt(s * s + rho2)
    for s0, s1 in ((-3.0, 3.0), (0.5, 40.0), (-1.0, -0.25)):
        want = np.asarray([3.0, 2.0, 1.0]) * (2 * e) ** 2 / (4 * np.pi) * (primitive(s1) - primitive(s0))
        got, err = _both(sc, sd, [s0, 0.0, z0], [1.0, 0.0, 0.0], s1 - s0, (1.0, 0.0, None))
        assert np.all(np.abs(got - want) <= err + 4e-6 * want), (s0, s1, got, want, err)
        assert np.all(err <= 5e-3 * want), (err, want)           # and the estimate is no blanket: half a percent, below any margin of the tests


def test_rectangle_on_its_axis_matches_the_solid_angle(built):
    """sigma_t -> 0, isotropic: what is left of the inner integral is the solid angle of the rectangle, on its axis
    4 atan(a b / (2 z sqrt(4 z^2 + a^2 + b^2))): the pure geometric factor.  The ray runs down the axis from 0.5 to 2.5 below a 1.0 x 0.6 light; the outer
    integral of the closed form is a midpoint rule of 200 000 cells."""
    a, b = 1.0, 0.6
    sd = _lone_light(a / 2, b / 2, 3.0, emission=(1.0, 1.0, 1.0))
    sc = orc.Scene(sd)
    z = 0.5 + (np.arange(200000) + 0.5) * (2.0 / 200000)
    want = np.sum(4.0 * np.arctan(a * b / (2.0 * z * np.sqrt(4.0 * z * z + a * a + b * b)))) * (2.0 / 200000) / (4 * np.pi)
    got, err = _both(sc, sd, [0.0, 2.5, 0.0], [0.0, -1.0, 0.0], 2.0, (1.0, 0.0, None))
    assert np.all(np.abs(got - want) <= err + 1e-9), (got, want, err)
    assert np.all(err <= 5e-3 * want), (err, want)


@pytest.mark.parametrize("g", [None, 0.7, -0.4])
def test_attenuated_point_light_matches_a_dense_rule(built, g):
    """sigma_t > 0 per channel, sigma_s != sigma_t, either phase function: the point-like light again, against a midpoint rule of 400 000 cells over
    sigma_s e^{-sigma_t (t + r)} p(cos) h / r^3, written out here on its own (forward scattering, cos = 1, is the light travelling along -d... towards the
    camera: cos = (x - y) . (-d) / r)."""
    e, h, z0 = 0.002, 1.5, 0.3
    sd = _lone_light(e, e, h)
    sc = orc.Scene(sd)
    sigma_s, sigma_t = np.asarray([0.4, 1.0, 1.5]), np.asarray([0.9, 1.2, 1.6])
    n, length = 400000, 5.0
    t = (np.arange(n) + 0.5) * (length / n)
    x = np.stack([-2.0 + t, np.zeros(n), np.full(n, z0)], axis=1)
    to_x = x - np.asarray([0.0, h, 0.0])
    r = np.linalg.norm(to_x, axis=1)
    cos = -to_x[:, 0] / r
    p = np.full(n, 1 / (4 * np.pi)) if g is None else (1 - g * g) / (4 * np.pi * (1 + g * g - 2 * g * cos) ** 1.5)
    want = np.asarray([3.0, 2.0, 1.0]) * (2 * e) ** 2 * np.asarray(
        [np.sum(sigma_s[c] * np.exp(-sigma_t[c] * (t + r)) * p * h / r ** 3) * (length / n) for c in range(3)])
    got, err = _both(sc, sd, [-2.0, 0.0, z0], [1.0, 0.0, 0.0], length, (sigma_s, sigma_t, g))
    assert np.all(np.abs(got - want) <= err + 4e-6 * want), (got, want, err)
    assert np.all(err <= 5e-3 * want), (err, want)           # and the estimate is no blanket: half a percent, below any margin of the tests


def test_the_tail_bound_bounds_the_tail(built):
    """A ray that runs on for ever under the lone light: the radiance beyond a cut of 30 units, by the rule itself on [30, 1e4], is below the closed-form
    bound, and the bound shrinks as e^{-sigma_t cut}."""
    sd = _lone_light(0.2, 0.2, 2.0, medium=scenes.Medium((0.0,) * 3, (0.025,) * 3))
    sc = orc.Scene(sd)
    o, d, far = np.asarray([[-3.0, 0.0, 0.0]]), np.asarray([[1.0, 0.0, 0.0]]), np.asarray([np.finfo(np.float32).max])
    bound = Q.tail_bound(sd, o, d, far, cut=30.0)[0]
    beyond = Q.radiance(sc, sd, o, d, far, 2)[0] - Q.radiance(sc, sd, o, d, far, 2, cut=30.0)[0]
    assert np.all(beyond > 0) and np.all(beyond <= bound), (beyond, bound)
    assert np.all(Q.tail_bound(sd, o, d, far)[0] < 1e-100)                       # at the cut the module uses


# ---- convergence on the scenes the tests use
def _box(sigma_s, sigma_a=0.0, g=None, w=W, h=H):
    return black_walls(scenes.cbox_medium(w, h, sigma_s, sigma_a, g))


@pytest.fixture(scope="module")
def rays(built):
    """The camera rays of seed 5 in the 12 x 9 box, and which of them are kept."""
    sd = _box(1.0)
    sc = orc.Scene(sd)
    px, py, o, d, tfar = B.camera_samples(sc, sd, orc.block_seeds(5, W, H), 1)
    return sd, sc, o, d, tfar, ~Q.near_a_light(sd, o, d, tfar, NEAR)


def test_doubling_the_resolution_moves_the_image_mean_by_less_than_two_in_a_thousand(rays):
    """Resolution 2 (the value the tests use) against resolution 4, over every medium of the tests below and of the GPU file at once: grey thick and thin,
    coloured with absorption, Henyey-Greenstein.  The error estimate (resolution 2 against 1) is no smaller than that step."""
    sd, sc, o, d, tfar, keep = rays
    media = [(1.0, 1.0, None), (0.025, 0.025, None), ((0.4, 1.0, 1.5), (0.9, 1.2, 1.6), None), (1.0, 1.0, 0.8), (0.1, 0.1, -0.5)]
    assert keep.mean() >= 0.9
    l1, l2, l4 = (Q.radiance(sc, sd, o[keep], d[keep], tfar[keep], res, media).mean(axis=1) for res in (1, 2, 4))
    step = np.abs(l4 - l2) / l4
    print("resolution 2 -> 4:", step.max(), " 1 -> 2:", (np.abs(l2 - l1) / l2).max())
    assert step.max() < 2e-3
    assert np.all(np.abs(l2 - l1) >= np.abs(l4 - l2))


def test_two_lights_converge_too(built):
    sd = black_walls(two_lights(W, H))
    sc = orc.Scene(sd)
    assert len(Q.lights_of(sd)) == 2
    px, py, o, d, tfar = B.camera_samples(sc, sd, orc.block_seeds(6, W, H), 1)
    keep = ~Q.near_a_light(sd, o, d, tfar, NEAR)
    assert keep.mean() >= 0.9
    l2, l4 = (Q.radiance(sc, sd, o[keep], d[keep], tfar[keep], res).mean(axis=0) for res in (2, 4))
    assert (np.abs(l4 - l2) / l4).max() < 2e-3


def test_the_phase_functions_are_told_apart(rays):
    """What the GPU file's Henyey-Greenstein cases rest on.  At g = -0.8 (the plane integrator's case, which must come out isotropic) the isotropic
    quadrature of the box is several times the HG one: further from it than ten times any margin the tests can allow (4 x 5 % + 1 % of quadrature error
    at the very most).  And negating g moves the HG quadrature by as much at g = -0.8, and by more than any such margin at the g = 0.6 of the other cases."""
    sd, sc, o, d, tfar, keep = rays
    media = [(1.0, 1.0, None), (1.0, 1.0, -0.8), (1.0, 1.0, 0.8), (1.0, 1.0, 0.6), (1.0, 1.0, -0.6)]
    iso, hg, neg, hg6, neg6 = Q.radiance(sc, sd, o[keep], d[keep], tfar[keep], 2, media).mean(axis=1)
    print("isotropic / HG(-0.8):", iso / hg, " HG(0.8) / HG(-0.8):", neg / hg, " HG(-0.6) / HG(0.6):", neg6 / hg6)
    assert np.all(np.abs(iso / hg - 1.0) > 10 * 0.21) and np.all(np.abs(neg / hg - 1.0) > 10 * 0.21), (iso / hg, neg / hg)
    assert np.all(np.abs(neg6 / hg6 - 1.0) > 0.21) and np.all(np.abs(iso / hg6 - 1.0) > 0.21), (neg6 / hg6, iso / hg6)


def test_the_photon_radius_biases_the_mean_by_less_than_half_a_percent(built):
    """The beam radiance estimate averages the radiance over a disc of the photon radius across the camera ray.  Bounded with the reference alone: on the
    24 x 18 frame of the GPU file, the image mean of the quadrature over rays moved by the radius along each of four directions across the ray stays within
    0.5 % of the unmoved rays' (the disc's average moves by less than its rim does), in the thin and in the thick medium the GPU file renders."""
    sd = _box(1.0, w=24, h=18)
    sc = orc.Scene(sd)
    px, py, o, d, tfar = B.camera_samples(sc, sd, orc.block_seeds(7, 24, 18), 1)
    keep = ~Q.near_a_light(sd, o, d, tfar, NEAR)
    o, d, tfar = o[keep].astype(np.float64), d[keep].astype(np.float64), tfar[keep]
    media = [(0.025, 0.025, None), (0.025, 0.025, 0.6), (1.0, 1.0, None)]
    e0 = np.cross(d, [0.0, 1.0, 0.0])
    e0 /= np.linalg.norm(e0, axis=1, keepdims=True)
    e1 = np.cross(d, e0)
    base = Q.radiance(sc, sd, o, d, tfar, 2, media).mean(axis=1)
    moved = np.mean([Q.radiance(sc, sd, o + Q.BRE_RADIUS * e, d, tfar, 2, media).mean(axis=1) for e in (e0, -e0, e1, -e1)], axis=0)
    print("radius", Q.BRE_RADIUS, "moves the mean by", np.abs(moved / base - 1.0).max(axis=1))
    assert np.abs(moved / base - 1.0).max() < 5e-3


# ---- the yardsticks at sizes the CPU affords
def _ratio(sc, sd, image, seeds, media=None):
    """(r [3], the quadrature's relative error [3]) of a 1 spp image against the quadrature on the rays those block seeds give."""
    px, py, o, d, tfar = B.camera_samples(sc, sd, seeds, 1)
    keep = ~Q.near_a_light(sd, o, d, tfar, NEAR)
    assert keep.mean() >= 0.9, "more than 10 % of the pixels masked"
    value, error = Q.image_mean(sc, sd, o, d, tfar, keep, media=media)
    return image[py, px][keep].mean(axis=0) / value, error / value


@pytest.mark.parametrize("strategy", ["ut", "cmis"])
def test_plane_single_restatement_agrees_with_the_quadrature(built, strategy):
    """1500 planes x 12 seeds in the grey box of sigma_s = 1 (the plane integrator ignores BSDFs)."""
    sd = scenes.cbox_medium(W, H, 1.0)
    sc = orc.Scene(sd)
    rs, es = [], []
    for k in range(12):
        run = P.compute(sd, seed=100 + k, nb_primitive=1500, strategy=strategy)
        r, e = _ratio(sc, sd, run["image"], run["seeds"])
        rs.append(r), es.append(e)
    Q.check_ratios(f"plane-single {strategy} restatement", rs, np.max(es, axis=0))


def test_bre_restatement_agrees_with_the_quadrature(built):
    """10 000 first-scatter photons x 8 seeds at sigma_s = 0.025, radius 0.05, black walls.  max_depth = 2 is the depth at which a light path stores its first
    medium vertex and nothing after it (every path walks one vertex, the light's: vertices == paths shot), so the photons carry single scattering alone."""
    sd = _box(0.025)
    sc = orc.Scene(sd)
    rs, es = [], []
    for k in range(8):
        run = B.compute(sd, seed=200 + k, nb_primitive=10000, max_depth=2, radius=Q.BRE_RADIUS)
        assert run["gen_stats"]["vertices"] == run["n_paths"] and run["records"].shape[0] <= run["n_paths"]
        r, e = _ratio(sc, sd, run["image"], run["seeds"])
        rs.append(r), es.append(e)
    Q.check_ratios("bre restatement", rs, np.max(es, axis=0))


@pytest.mark.parametrize("g", [None, 0.6])
def test_oracle_path_tracer_agrees_with_the_quadrature(built, g):
    """path with max_depth = 3, min_depth = 1, strategy = emitter on black walls: camera -> medium vertex -> light and nothing else (max_depth = 2 is
    black, asserted).  1024 spp x 8 seeds at sigma_s = 0.05 (at sigma_s = 1 the 5.8 units in front of the box leave e^-6 of the signal); so many samples
    average the jitter out, and the reference is the radiance integrated over each pixel's footprint."""
    sd = _box(0.05, g=g)
    sc = orc.Scene(sd)
    ref = Q.Footprint(sc, sd, 2, NEAR)
    assert ref.keep.mean() >= 0.9
    value, error = (v[0] for v in ref.mean())
    assert not sc.render(master_seed=1, spp=4, max_depth=2, min_depth=1, strategy=api.STRATEGY_EMITTER, stream_mode=1)[0].any()
    rs = [sc.render(master_seed=300 + k, spp=1024, max_depth=3, min_depth=1, strategy=api.STRATEGY_EMITTER, stream_mode=1)[0][ref.keep].mean(axis=0)
          / value for k in range(8)]
    Q.check_ratios(f"oracle path g = {g}", rs, error / value)
