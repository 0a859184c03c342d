"""IntegratorLightTracing (rl_render_light, kernels/light.hip.h): the light tracer against the furnace's closed form and against the path tracer
(statistically, from the seed-to-seed spread), its exact rules (depth, smooth surfaces, strategies, counters), bit-determinism across execution forms,
its refusals and the CLI end to end.  At most one child process at a time."""
import os
import subprocess

import numpy as np
import pytest

from rustlight_amd import api, scenes
from tests import cli

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 10          # independent seeds per estimate


def _seeds(k, w, h):
    return api.IndependentSampler(1000 + 17 * k).block_seeds(w, h)


def _block_means(img, b):
    h, w = img.shape[:2]
    lum = img.astype(np.float64).mean(axis=2)
    return lum[: h // b * b, : w // b * b].reshape(h // b, b, w // b, b).mean(axis=(1, 3))


def _estimates(render, w, h, b, offset=0):
    """R independent renders -> (mean, standard error) of the b x b block means."""
    m = np.stack([_block_means(render(_seeds(offset + k, w, h)), b) for k in range(R)])
    return m.mean(axis=0), m.std(axis=0, ddof=1) / np.sqrt(R)


def _compare_with_path(sd, spp_light, spp_path, strategy_path=api.STRATEGY_ALL, min_depth=0, max_depth=None):
    """light(min, max) against path(min, max + 1): a light vertex at evaluation depth d closes a path of d + 1 segments and exists up to d = max - 1,
    while `path` adds emission over segments 1 .. max - 1 (its vertex at generate depth g is expanded when g < max).  min_depth means the same in both."""
    ctx = api.Context(api.Scene(sd), 0)
    w, h = sd.width, sd.height
    ml, sl = _estimates(lambda s: ctx.render_light(s, spp=spp_light, min_depth=min_depth, max_depth=max_depth)[0], w, h, 8)
    pmax = None if max_depth is None else max_depth + 1
    mp, sp = _estimates(lambda s: ctx.render(s, api.path_params(spp_path, min_depth=min_depth, max_depth=pmax, strategy=strategy_path,
                                                                  stream_mode=api.STREAM_PER_SAMPLE))[0], w, h, 8, offset=100)
    se = np.sqrt(sl ** 2 + sp ** 2)
    lit = mp > 1e-3
    assert lit.mean() > 0.5
    z = (ml - mp) / np.where(se > 0, se, 1.0)
    assert np.all(np.abs(z[se > 0]) < 5.0), (np.abs(z).max(), ml, mp)
    assert np.all(ml[se == 0] == mp[se == 0])
    return ml, mp


def test_furnace(built):
    sd = scenes.furnace(albedo=0.5)
    ctx = api.Context(api.Scene(sd), 0)
    imgs = np.stack([ctx.render_light(_seeds(k, sd.width, sd.height), spp=8)[0] for k in range(R)]).astype(np.float64)
    means = imgs.mean(axis=(1, 2, 3))
    se = means.std(ddof=1) / np.sqrt(R)
    assert abs(means.mean() - 2.0) < 4.0 * se, (means.mean(), se)
    blocks = np.stack([_block_means(i, 4) for i in imgs])
    bse = blocks.std(axis=0, ddof=1) / np.sqrt(R)
    assert np.all(np.abs(blocks.mean(axis=0) - 2.0) < 5.0 * bse), np.abs((blocks.mean(axis=0) - 2.0) / bse).max()


def test_cbox_default_depths(built):
    _compare_with_path(scenes.cbox(64, 64), 16, 16)


def test_cbox_min1_max3(built):
    _compare_with_path(scenes.cbox(64, 64), 16, 16, min_depth=1, max_depth=3)


def test_cbox_medium(built):
    # Acceleration::visible calls a segment that misses the scene's root box occluded (accel.rs:338-340): a medium vertex outside the box could then never
    # reach the camera, which sits outside the Cornell box.  A small triangle behind the camera stretches the root box over the camera and the medium in
    # front of it, so that both integrators see the same transport.
    sd = scenes.cbox_medium(64, 64, 0.5)
    back = scenes.MeshData("Back", np.asarray([[0.0, 1.0, 8.0], [0.01, 1.0, 8.0], [0.0, 1.01, 8.0]], dtype=np.float32), np.asarray([[0, 1, 2]], dtype=np.uint32),
                           None, None, scenes.matte((0.5, 0.5, 0.5)))
    sd.meshes.insert(0, back)
    _compare_with_path(sd, 16, 16, max_depth=6)


def test_cbox_point_and_directional(built):
    _compare_with_path(scenes.cbox_other_lights(64, 64, environment=False), 16, 16)


def test_cbox_hsv_emission(built):
    # the HSV colour of a SAMPLED light point comes from its normalised uv (geometry.rs:316-325), that of a light HIT from the hit's uv: the light
    # tracer samples every emission, so it is compared with the path tracer's light-sampling strategy and without the directly seen light
    sd = scenes.override_light_emission(scenes.cbox(64, 64), "hsv")
    _compare_with_path(sd, 16, 16, strategy_path=api.STRATEGY_EMITTER, min_depth=1)


def test_max_depth_one_is_black(built):
    sd = scenes.cbox(32, 32)
    img, st = api.Context(api.Scene(sd), 0).render_light(_seeds(0, 32, 32), spp=4, max_depth=1)
    assert not img.any()
    assert st["camera_samples"] == 4 * 32 * 32 and st["splats"] == 0 and st["shadow_rays"] == 0


def _mirror_scene():
    sd = scenes.cbox(64, 64)
    n = np.array([0.5, 0.0, 0.866]); n /= np.linalg.norm(n)
    t = np.array([0.0, 1.0, 0.0]); bt = np.cross(t, n)
    c = np.array([0.0, 1.0, 0.0])
    P = [c + a * 0.25 * bt + b * 0.25 * t for a, b in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
    mirror = scenes.Bsdf(type=scenes.METAL, specular=scenes.const_color((1, 1, 1)), distribution=scenes.MF_NONE)
    sd.meshes.insert(0, scenes._quad_mesh("Mirror", [float(x) for p in P for x in p], [float(x) for x in n], mirror))
    return sd


def test_smooth_surfaces_are_never_camera_connections(built):
    sd = _mirror_scene()
    scene = api.Scene(sd)
    ctx = api.Context(scene, 0)
    o, d = zip(*[scene.camera_ray(x + 0.5, y + 0.5) for y in range(sd.height) for x in range(sd.width)])
    _, _, _, mesh, _ = ctx.trace(np.array(o), np.array(d))
    on_mirror = (mesh == 0).reshape(sd.height, sd.width)
    assert 50 < on_mirror.sum() < sd.width * sd.height // 2
    # the pixels around the mirror's outline may also receive splats through their other half: look at pixels whose four neighbours are mirror too
    inner = on_mirror.copy()
    inner[1:-1, 1:-1] &= on_mirror[:-2, 1:-1] & on_mirror[2:, 1:-1] & on_mirror[1:-1, :-2] & on_mirror[1:-1, 2:]
    inner[[0, -1], :] = False; inner[:, [0, -1]] = False
    light = ctx.render_light(_seeds(0, 64, 64), spp=16)[0]
    path = ctx.render(_seeds(0, 64, 64), api.path_params(16))[0]
    assert inner.sum() > 20
    assert not light[inner].any()
    assert (path[inner].sum(axis=-1) > 0).mean() > 0.9


def test_surface_plus_volume_is_all(built):
    sd = scenes.cbox_medium(48, 48, 0.5)
    ctx = api.Context(api.Scene(sd), 0)
    s = _seeds(3, 48, 48)
    a, sa = ctx.render_light(s, spp=8, strategy=api.LIGHT_ALL)
    su, ss = ctx.render_light(s, spp=8, strategy=api.LIGHT_SURFACE)
    vo, sv = ctx.render_light(s, spp=8, strategy=api.LIGHT_VOLUME)
    assert su.any() and vo.any()
    assert sa["rng_draws"] == ss["rng_draws"] == sv["rng_draws"] and sa["extension_rays"] == ss["extension_rays"] == sv["extension_rays"]
    assert sa["splats"] == ss["splats"] + sv["splats"]
    np.testing.assert_allclose(a, su.astype(np.float64) + vo, rtol=1e-6, atol=0)


def test_counters(built):
    sd = scenes.cbox(64, 64)
    spp = 8
    img, st = api.Context(api.Scene(sd), 0).render_light(_seeds(1, 64, 64), spp=spp)
    assert st["camera_samples"] == spp * 64 * 64
    assert st["kernel_launches"] == 3 and st["ms_other"] > 0
    assert 0 < st["splats"] and st["splats"] + st["splats_invalid"] <= st["shadow_rays"]
    assert st["splats_invalid"] == 0 and st["splats_saturated"] == 0
    assert st["vertices"] >= st["camera_samples"] and st["extension_rays"] >= st["camera_samples"]
    assert st["rng_draws"] >= 6 * st["camera_samples"]
    assert np.isfinite(img).all() and img.min() >= 0.0


def test_deterministic(built, monkeypatch):
    sd = scenes.cbox_medium(48, 48, 0.3)
    s = _seeds(5, 48, 48)
    monkeypatch.delenv("RL_FORCE_STREAMING", raising=False)
    ctx = api.Context(api.Scene(sd), 0)
    a = ctx.render_light(s, spp=8)[0]
    b = ctx.render_light(s, spp=8)[0]
    assert a.tobytes() == b.tobytes()
    monkeypatch.setenv("RL_FORCE_STREAMING", "1")
    c = api.Context(api.Scene(sd), 0).render_light(s, spp=8)[0]
    monkeypatch.delenv("RL_FORCE_STREAMING", raising=False)
    assert a.tobytes() == c.tobytes()
    d = ctx.render_light(_seeds(6, 48, 48), spp=8)[0]
    assert a.tobytes() != d.tobytes()


def test_refusals(built):
    ctx = api.Context(api.Scene(scenes.cbox(32, 32)), 0)
    s = _seeds(0, 32, 32)
    for kw in ({"stream_mode": api.STREAM_REFERENCE_ORDER}, {"stream_mode": api.STREAM_STRATIFIED}, {"numerics": api.NUMERICS_FAST}, {"shard_count": 2}):
        with pytest.raises(api.RustlightError) as e:
            ctx.render_light(s, spp=1, **kw)
        assert e.value.code == api.RL_ERR_UNSUPPORTED, kw
    sky = api.Context(api.Scene(scenes.sky_scene(32, 32)), 0)
    with pytest.raises(api.RustlightError) as e:
        sky.render_light(s, spp=1)
    assert e.value.code == api.RL_ERR_UNSUPPORTED and "environment" in str(e.value)
    dark = scenes.cbox(32, 32)
    dark.meshes[-1].emission = None
    with pytest.raises(api.RustlightError) as e:
        api.Context(api.Scene(dark), 0).render_light(s, spp=1)
    assert e.value.code == api.RL_ERR_NO_EMITTER


def test_cli_renders_what_the_api_renders(built, tmp_path):
    scn = os.path.join(ROOT, "data", "cbox.pbrt")
    out = str(tmp_path / "out.pfm")
    r = subprocess.run([cli.EXE, scn, "-n", "4", "-r", "independent:7", "-o", out, "light-tracing"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img = api.load_pfm(out)
    want = api.IntegratorLightTracing().compute(api.IndependentSampler(7), api.Scene.load(scn), 4)
    assert img.shape == want.shape and want.any()
    np.testing.assert_array_equal(img, want)
