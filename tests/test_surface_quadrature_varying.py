"""What tests/surface_quadrature.py says of textures, of lights whose emission depends on uv and of the environment map, held to closed forms it shares no
code with; and then every case of tests/test_gpu_surface_quadrature_varying.py on the CPU oracle, with the same seeds, counts and check
(tests/surface_varying_cases.py).  The oracle is bit-identical to the device, so what holds or misses here holds or misses there; the figures of both are
in profiles/surface_varying_note.md."""
import numpy as np
import pytest

from oracle import orc
from rustlight_amd import scenes
from tests import surface_quadrature as Q
from tests import surface_varying_cases as C
from tests.scene_helpers import RECEIVER_ALBEDO, RECEIVERS, open_floor, ray_at_receiver as _ray_at_receiver, receiver_scene as _receiver_scene

W, H = C.W, C.H
ALBEDO = np.asarray(RECEIVER_ALBEDO)


def _pixel_centres(sc, step=3):
    return tuple(np.asarray(a) for a in zip(*[sc.camera_generate(x + 0.5, y + 0.5) for y in range(0, H, step) for x in range(0, W, step)]))


# ---- textures
def _floor_radiance(diffuse, bitmaps=()):
    sd = open_floor(W, H, bsdf=scenes.Bsdf(type=scenes.DIFFUSE, diffuse=diffuse))
    sd.bitmaps = list(bitmaps)
    sc = orc.Scene(sd)
    return Q.radiance(sc, sd, *_pixel_centres(sc), 1)


def test_textures_of_one_colour_are_the_constant_texture(built):
    """A checkerboard and a grid whose two colours are equal, and a bitmap of one texel, read the constant case to 1e-12."""
    colour = (0.7, 0.5, 0.3)
    want = _floor_radiance(scenes.const_color(colour))
    assert want.max() > 0.0
    for kind in (scenes.TEX_CHECKERBOARD, scenes.TEX_GRID):
        tex = {"type": kind, "color0": colour, "color1": colour, "scale": (4.0, 3.0), "offset": (0.1, 0.2), "line_width": 0.1}
        np.testing.assert_allclose(_floor_radiance(tex), want, rtol=1e-12)
    bitmap = (1, 1, np.asarray([[colour]], np.float32))
    got = _floor_radiance({"type": scenes.TEX_BITMAP, "color0": (0.0, 0.0, 0.0), "bitmap_id": 0}, [bitmap])
    np.testing.assert_allclose(got, want * (np.asarray(colour, np.float32).astype(np.float64) / colour), rtol=1e-12)


def test_the_textures_at_known_points():
    """The checkerboard's sign product, the grid's lines under both readings of scale_v, the bitmap's nearest texel and its wrap, and no uv."""
    c0, c1 = np.asarray([1.0, 0.0, 0.0]), np.asarray([0.0, 0.0, 1.0])
    checker = {"type": scenes.TEX_CHECKERBOARD, "color0": tuple(c0), "color1": tuple(c1), "scale": (2.0, 2.0), "offset": (0.0, 0.0)}
    uv = np.asarray([[0.1, 0.1], [0.3, 0.1], [0.3, 0.3], [0.6, 0.3], [0.1, np.nan]])                # 2 uv * 2: halves (0, 0), (1, 0), (1, 1), (2, 1)
    np.testing.assert_array_equal(Q.texture(checker, uv), [c0, c1, c0, c1, [0.0, 0.0, 0.0]])
    np.testing.assert_array_equal(Q.texture(checker, None), [0.0, 0.0, 0.0])
    grid = {"type": scenes.TEX_GRID, "color0": tuple(c0), "color1": tuple(c1), "scale": (4.0, 0.45), "offset": (0.0, 0.0), "line_width": 0.1}
    uv = np.asarray([[0.51, 0.3], [0.4, 0.5], [0.4, 0.3]])                                          # 4 u = 2.04: a line; v + 0.45 = 0.95: a line under "added" alone
    np.testing.assert_array_equal(Q.texture(grid, uv, departures=Q.REFERENCE), [c0, c0, c1])
    np.testing.assert_array_equal(Q.texture(grid, uv, departures=Q.PUBLISHED), [c0, c1, c1])
    rgb = np.arange(18, dtype=np.float32).reshape(2, 3, 3)                                           # 3 x 2 texels, texel (x, y) holds 9 y + 3 x + (0, 1, 2)
    tex = {"type": scenes.TEX_BITMAP, "color0": (0.0, 0.0, 0.0), "bitmap_id": 0}
    uv = np.asarray([[0.1, 0.1], [0.5, 0.1], [0.9, 0.6], [1.4, -0.4], [-0.1, 2.7]])                 # texels (0, 0), (1, 0), (2, 1), (1, 1), (2, 1)
    np.testing.assert_array_equal(Q.texture(tex, uv, [(3, 2, rgb)])[:, 0], [0.0, 3.0, 15.0, 12.0, 15.0])


def test_hits_carry_the_uv_of_the_point(built):
    """The uv interpolated with the oracle's barycentrics is, on the box's floor (uv (0, 0), (1, 0), (1, 1), (0, 1) on its corners), the hit point's affine
    image: the barycentrics are (1 - u - v, u, v) on the triangle's corners in order."""
    sd = scenes.cbox(W, H)
    sc = orc.Scene(sd)
    hits = Q.Hits(sc, sd, *_pixel_centres(sc, 1))
    floor = hits.mesh == 0
    assert floor.sum() >= 8
    corner = np.asarray(sd.meshes[0].vertices, np.float64).reshape(4, 3)
    e0, e1 = corner[1] - corner[0], corner[3] - corner[0]
    rel = hits.p[floor] - corner[0]
    want = np.stack([rel @ e0 / (e0 @ e0), rel @ e1 / (e1 @ e1)], axis=-1)
    np.testing.assert_allclose(hits.uv[floor], want, atol=2e-6)
    sd = scenes.single_triangle()                                       # a mesh without uv
    assert np.isnan(Q.Hits(orc.Scene(sd), sd, [[0.25, 0.25, -3.0]], [[0.0, 0.0, 1.0]]).uv).all()


# ---- lights whose emission depends on uv
def _uv_light(kind, quad=(0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 1.0), bitmaps=()):
    mesh = scenes._quad_mesh("light", list(quad), [0, -1, 0], scenes.matte((0, 0, 0)), emission=(1.0, 1.0, 1.0))
    mesh.emission_kind = kind
    return Q.UvLight(mesh, bitmaps)


M_NORMALISED = (np.sqrt(2.0) + np.arcsinh(1.0) - 1.0) / 2.0        # the mean of u / |uv| over the unit square: int cos(theta) r dr dtheta over its two triangles


def test_the_mean_of_hsv_over_the_unit_square():
    """Under true uv (0.5, 0.5, 0) scale, exactly; under normalised uv (m, 1 - m, 0) scale with m = 0.64779.  The integrand is bounded and smooth but at
    the uv origin, where its limit depends on the direction: the panelled rule holds it to 2e-4 at 16 x 16 panels of 4 x 4 nodes."""
    light = _uv_light(("hsv", 3.0))
    a, b = Q._panel_ab(16, 4)
    _, w = Q._panel_grid(light, 16, 4)
    assert light.area == pytest.approx(1.0, abs=1e-12)
    np.testing.assert_allclose(w @ light.le(a, b, False), [1.5, 1.5, 0.0], atol=1e-12)
    np.testing.assert_allclose(w @ light.le(a, b, True), [3.0 * M_NORMALISED, 3.0 * (1.0 - M_NORMALISED), 0.0], atol=6e-4)
    np.testing.assert_allclose(w @ light.le(a, b, True, Q.PUBLISHED), [1.5, 1.5, 0.0], atol=1e-12)
    assert abs(M_NORMALISED - 0.64779) < 1e-5


def test_the_texture_light_by_texel():
    """A 2 x 2 bitmap: under true uv each texel covers a quarter; under normalised uv the unit circle's arc from (1, 0) to (0, 1) crosses u = 0.5 at 60 and
    v = 0.5 at 30 degrees, so texel (1, 0) covers tan(30) / 2 of the square, (0, 1) the same, (1, 1) the rest and (0, 0) nothing."""
    rgb = np.asarray([[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], [[0.0, 0.0, 1.0], [1.0, 1.0, 1.0]]], np.float32)      # (0, 0) red, (1, 0) green, (0, 1) blue, (1, 1) white
    light = _uv_light(("texture", 2.0, 0), bitmaps=[(2, 2, rgb)])
    a, b = Q._panel_ab(64, 2)
    _, w = Q._panel_grid(light, 64, 2)
    np.testing.assert_allclose(w @ light.le(a, b, False), 2.0 * np.asarray([0.5, 0.5, 0.5]), atol=1e-12)
    side = np.tan(np.radians(30.0)) / 2.0
    np.testing.assert_allclose(w @ light.le(a, b, True), 2.0 * np.asarray([1.0 - 2.0 * side, 1.0 - side, 1.0 - side]), atol=2e-3)
    _, w, a, b = light.sector_grid(1, 2)                                 # the rule that follows those rays: exact, and its weights are the quad's area
    np.testing.assert_allclose(w @ light.le(a, b, True), 2.0 * np.asarray([1.0 - 2.0 * side, 1.0 - side, 1.0 - side]), atol=1e-12)
    assert w.sum() == pytest.approx(light.area, abs=1e-12) and a.min() > 0.0 and a.max() < 1.0 and b.min() > 0.0 and b.max() < 1.0
    np.testing.assert_allclose(w @ np.stack([a, b, a * b], axis=-1), [0.5, 0.5, 0.25], atol=1e-12)


@pytest.mark.parametrize("which", ["bsdf", "emitter", "all"])
def test_the_far_field_of_a_small_uv_light(built, which):
    """A 0.004 x 0.004 HSV quad is a point light of intensity mean(Le) A cos_l: albedo / pi mean(Le) A cos_x cos_l / r^2, with the mean of the emission the
    strategy integrates.  Le runs over its whole range across the quad and the geometry term over about 2 size / r of its value, so their covariance, what
    the product of the means leaves out, is within 2 size / r; the rule's own share is 1e-4, or 2e-3 where Le is not smooth.  Mixed, the two means under
    weights that sum to one lie between them."""
    e, scale = 0.002, 3.0
    quad = [-e, 2.0, -e, e, 2.0, -e, e, 2.0, e, -e, 2.0, e]
    mean = {"bsdf": np.asarray([0.5, 0.5, 0.0]), "emitter": np.asarray([M_NORMALISED, 1.0 - M_NORMALISED, 0.0])}
    for i, (p, n) in enumerate(RECEIVERS):
        sd = _receiver_scene(i, quad)
        sd.meshes[0].emission_kind = ("hsv", scale)
        got = Q.radiance(orc.Scene(sd), sd, *_ray_at_receiver(i), 4, lights=which)[0]
        n = np.asarray(n) / np.linalg.norm(n)
        r = np.asarray([0.0, 2.0, 0.0]) - np.asarray(p)
        dist = np.linalg.norm(r)
        geometry = ALBEDO / np.pi * scale * (2 * e) ** 2 * (n @ r / dist) * (r[1] / dist) / dist ** 2
        if which == "all":
            low, high = np.minimum(mean["bsdf"], mean["emitter"]), np.maximum(mean["bsdf"], mean["emitter"])
            slack = 2.0 * (2 * e) / dist + 2e-3
            assert np.all(got >= geometry * low * (1.0 - slack)) and np.all(got <= geometry * high * (1.0 + slack)), (i, got)
            assert got[2] == 0.0
        else:
            np.testing.assert_allclose(got, geometry * mean[which], rtol=2.0 * (2 * e) / dist + (2e-3 if which == "emitter" else 1e-4), atol=1e-15)


# ---- the environment map
def _patch_under_a_map(env, normal_up="z"):
    """A small triangle at the origin, alone, whose normal is +z (or +y), under the map; a ray straight down its normal."""
    tri = {"z": [[0.01, 0.0, 0.0], [-0.005, 0.009, 0.0], [-0.005, -0.009, 0.0]], "y": [[0.01, 0.0, 0.0], [-0.005, 0.0, -0.009], [-0.005, 0.0, 0.009]]}[normal_up]
    mesh = scenes.MeshData("patch", np.asarray(tri, np.float32), np.asarray([[0, 1, 2]], np.uint32), None, None, scenes.matte(tuple(ALBEDO)))
    to_world = np.asarray([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, -5, 1], dtype=np.float32)
    sd = scenes.SceneData(8, 8, 40.0, 0, to_world, False, [mesh])
    sd.environment_map = np.asarray(env, np.float32)
    up = np.asarray({"z": [0.0, 0.0, 1.0], "y": [0.0, 1.0, 0.0]}[normal_up])
    return sd, (0.3 * up)[None, :], (-up)[None, :]


def test_a_patch_under_a_map(built):
    """Unoccluded, normal +z: the irradiance is the sum over the upper texels of Le (phi_1 - phi_0) (cos^2 theta_0 - cos^2 theta_1) / 2, which the rule
    integrates exactly (cos_x is cos(theta)); as a sampled direction and as a light sample find it under the published model alike.  A map of one colour is
    the constant sky, to 1e-12."""
    env = np.random.default_rng(3).uniform(0.1, 2.0, (4, 8, 3)).astype(np.float32)
    sd, o, d = _patch_under_a_map(env)
    sc = orc.Scene(sd)
    h, w = env.shape[:2]
    want = np.zeros(3)
    for row in range(h // 2):
        for col in range(w):
            want += env[row, col].astype(np.float64) * (2.0 * np.pi / w) * (np.cos(row * np.pi / h) ** 2 - np.cos((row + 1) * np.pi / h) ** 2) / 2.0
    for res in (1, 2):
        np.testing.assert_allclose(Q.radiance(sc, sd, o, d, res)[0], ALBEDO / np.pi * want, rtol=1e-12)
        np.testing.assert_allclose(Q.radiance(sc, sd, o, d, res, sky="emitter", departures=Q.PUBLISHED)[0], ALBEDO / np.pi * want, rtol=1e-12)
    colour = (0.3, 0.4, 0.6)
    sd, o, d = _patch_under_a_map(np.tile(np.asarray(colour, np.float32), (4, 8, 1)))
    got = Q.radiance(orc.Scene(sd), sd, o, d, 1)[0]
    sd.environment_map, sd.environment = None, colour
    np.testing.assert_allclose(got, Q.radiance(orc.Scene(sd), sd, o, d, 1)[0] * (np.asarray(colour, np.float32).astype(np.float64) / colour), rtol=1e-12)
    np.testing.assert_allclose(got, ALBEDO * np.asarray(colour, np.float32).astype(np.float64), rtol=1e-12)


def test_the_last_row_of_the_map_as_a_light_sample(built):
    """sky_last_bin = "edge" on the same patch turned to +y, which sees half of every row: the rows but the last are integrated as before, and the last
    row enters as sin(theta_0) pi / h at theta_0 = pi (h - 1) / h, the last column at phi_0; written out here for a map that is black but for one texel
    of the last row: E = Le sin(theta_0) (pi / h) sin(theta_0) int sin(phi) dphi over the texel."""
    h, w = 4, 8
    env = np.zeros((h, w, 3), np.float32)
    env[h - 1, 1] = (1.0, 2.0, 3.0)                                     # phi in 45 .. 90 degrees: y > 0
    sd, o, d = _patch_under_a_map(env, "y")
    sc = orc.Scene(sd)
    theta0 = np.pi * (h - 1) / h
    edge = np.sin(theta0) * (np.pi / h) * np.sin(theta0) * (np.cos(np.pi / 4.0) - np.cos(np.pi / 2.0))
    exact = (np.cos(np.pi / 4.0) - np.cos(np.pi / 2.0)) * (np.pi / h / 2.0 - (np.sin(2.0 * np.pi) - np.sin(2.0 * theta0)) / 4.0)     # int sin^2(theta) dtheta
    colour = np.asarray([1.0, 2.0, 3.0])
    np.testing.assert_allclose(Q.radiance(sc, sd, o, d, 2, sky="emitter")[0], ALBEDO / np.pi * colour * edge, rtol=1e-9)
    # sin(theta) = sqrt(1 - mu^2) has a root's singularity at the pole, where Gauss-Legendre in mu gains three orders per doubling only: 2e-3 at res 4
    np.testing.assert_allclose(Q.radiance(sc, sd, o, d, 4, sky="bsdf")[0], ALBEDO / np.pi * colour * exact, rtol=2e-3)
    np.testing.assert_allclose(Q.radiance(sc, sd, o, d, 4, sky="emitter", departures=Q.PUBLISHED)[0], ALBEDO / np.pi * colour * exact, rtol=2e-3)
    assert edge > 1.5 * exact


def test_the_direction_convention_of_the_map():
    """z up, no transform: +x is phi = 0 (column 0), +y a quarter turn on (column w / 4), +z row 0 and -z the last row."""
    env = np.random.default_rng(5).uniform(0.1, 2.0, (4, 8, 3))
    d = Q._unit(np.asarray([[1.0, 0.1, 0.1], [0.1, 1.0, 0.1], [0.2, 0.1, 1.0], [0.2, 0.1, -1.0], [1.0, -0.1, -0.1]]))
    np.testing.assert_array_equal(Q.sky_radiance(env, d), [env[1, 0], env[1, 1], env[0, 0], env[3, 0], env[2, 7]])
    density, mean = Q.sky_map_density(env)
    assert density.mean() == pytest.approx(1.0, abs=1e-12) and mean == pytest.approx(((env @ Q.LUMINANCE) * np.sin((np.arange(4) + 0.5) * np.pi / 4)[:, None]).mean())


def test_the_small_map_keeps_its_features():
    """scenes.sky_map(8, 4): a bright texel above the floor's horizon (y > 0), a black row and a black column."""
    env = scenes.sky_map(*C.SKY_MAP)
    assert env.shape == (4, 8, 3) and not env[1].any() and not env[:, 3].any()
    assert env[2, 2, 0] == 40.0 and np.sin((2 + 0.5) * 2.0 * np.pi / 8) > 0.0
    assert env[3, 0].all()                                                # the last row is lit: sky_last_bin shows


# ---- every case of the device's file on the oracle
@pytest.fixture(scope="module")
def references(built):
    return C.References()


@pytest.fixture(scope="module")
def oracle(built):
    return C.Oracle()


@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_oracle(references, oracle, case):
    C.run(case, oracle, references)
