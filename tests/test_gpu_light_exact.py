"""IntegratorLightTracing (rl_render_light, kernels/light.hip.h) held to the CPU oracle's light tracer (oracle/rl_oracle.cpp: orc_render_light, written
from src/integrators/explicit/light.rs): image bits and every counter both sides report, over scenes that reach each instantiation of k_light_fused,
the depth and strategy options, ragged and split-1 frame sizes, lane splits, LDS-staged and streamed scenes and both seed variants.  The edges of
the fixed-point splat image — invalid, saturated, overflowing and dim splats — are held to the oracle's f64 sums as well.  One process, no child."""
import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests.scene_helpers import context as _context, glass_and_mirror as _glass_and_mirror, single_bsdf as _single_bsdf, with_back_triangle as _with_back_triangle

pytestmark = pytest.mark.gpu

KEYS = ("camera_samples", "vertices", "extension_rays", "shadow_rays", "rng_draws", "splats", "splats_invalid", "splats_saturated")


def _seeds(sd, k, variant=0):
    return api.IndependentSampler(300 + k, variant).block_seeds(sd.width, sd.height)


def _exact(sd, ctx=None, seed=0, want_f64=False, streaming=False, **kw):
    """GPU and oracle: the same image bits and the same counters.  Returns (image, stats[, f64 sums, per-pixel splat counts])."""
    ctx = ctx or _context(sd, streaming)
    seeds = _seeds(sd, seed, kw.get("seed_variant", 0))
    img, st = ctx.render_light(seeds, **kw)
    got = orc.Scene(sd).render_light(seeds=seeds, want_f64=want_f64, **kw)
    ref, ost = got[0], got[1]
    for k in KEYS:
        assert st[k] == ost[k], (k, st[k], ost[k])
    np.testing.assert_array_equal(img, ref)
    assert st["camera_samples"] == kw.get("spp", 1) * sd.width * sd.height
    return (img, st) + tuple(got[2:])


def _exercised(img, st, counter="splats"):
    assert img.any() and st["splats"] > 0 and st[counter] > 0, (counter, st)


def _scene(name, w=24, h=24):
    if name == "cbox": return scenes.cbox(w, h)
    if name == "medium_g0.6": return _with_back_triangle(scenes.cbox_medium(w, h, 0.5, g=0.6))
    if name == "medium_g-0.3": return _with_back_triangle(scenes.cbox_medium(w, h, 0.5, 0.1, g=-0.3))
    if name == "point": return scenes.cbox_other_lights(w, h, point=True, directional=False, environment=False, keep_area_light=False)
    if name == "directional": return scenes.cbox_other_lights(w, h, point=False, directional=True, environment=False, keep_area_light=False)
    if name == "hsv": return scenes.override_light_emission(scenes.cbox(w, h), "hsv")
    if name == "texture":
        sd = scenes.cbox(w, h)
        sd.bitmaps.append((4, 3, np.random.default_rng(2).uniform(0.0, 2.0, (12, 3)).astype(np.float32)))
        return scenes.override_light_emission(sd, "texture", bitmap_id=0)
    if name == "mixed": return scenes.living_room(w + 8, h, n_spheres=8, tess=6)
    if name == "diffuse": return _single_bsdf(w, h, scenes.matte((0.6, 0.5, 0.4)))
    if name == "phong": return _single_bsdf(w, h, scenes.living_room_materials()[1])
    if name == "rough_metal": return _single_bsdf(w, h, scenes.Bsdf(type=scenes.METAL, specular=scenes.const_color((0.9, 0.8, 0.7)), distribution=scenes.MF_GGX, alpha_u=0.3, alpha_v=0.3))
    if name == "substrate": return _single_bsdf(w, h, scenes.living_room_materials()[5])
    if name == "glass_mirror": return _glass_and_mirror(w, h)
    raise KeyError(name)


SCENES = ["cbox", "medium_g0.6", "medium_g-0.3", "point", "directional", "hsv", "texture", "mixed", "diffuse", "phong", "rough_metal", "substrate", "glass_mirror"]


@pytest.mark.parametrize("name", SCENES)
def test_scenes_match_oracle(built, name):
    """Every scene kind, both scene placements, both seed variants; spp 3 (split > 1: uneven lanes on a small frame)."""
    sd = _scene(name)
    for streaming in (False, True):
        ctx = _context(sd, streaming)
        for variant in (0, 1):
            img, st = _exact(sd, ctx, seed=variant, spp=3, seed_variant=variant, max_depth=8 if name == "glass_mirror" else None)
            _exercised(img, st)
    if name.startswith("medium"):
        _exercised(*_exact(sd, ctx, seed=4, spp=3, strategy=api.LIGHT_VOLUME))


@pytest.mark.parametrize("kw", [dict(max_depth=1), dict(max_depth=2), dict(max_depth=3), dict(min_depth=2, max_depth=5), dict(rr_depth=0),
                                dict(rr_depth=None), dict(min_depth=None, max_depth=4, rr_depth=2), dict(rr_depth=0, max_depth=None)])
def test_depth_options_match_oracle(built, kw):
    for name in ("cbox", "medium_g0.6"):
        sd = _scene(name)
        img, st = _exact(sd, seed=7, spp=2, **kw)
        if kw.get("max_depth") == 1:
            assert not img.any() and st["splats"] == 0 and st["vertices"] == 0
        else:
            _exercised(img, st)


@pytest.mark.parametrize("strategy", [api.LIGHT_ALL, api.LIGHT_SURFACE, api.LIGHT_VOLUME])
def test_strategies_match_oracle(built, strategy):
    for name in ("cbox", "medium_g-0.3"):
        sd = _scene(name)
        img, st = _exact(sd, seed=8, spp=2, strategy=strategy)
        if strategy == api.LIGHT_VOLUME and name == "cbox":
            assert not img.any() and st["splats"] == 0
        else:
            _exercised(img, st)


@pytest.mark.parametrize("w,h,spp", [(5, 7, 1), (5, 7, 16), (33, 17, 3), (33, 17, 5), (16, 16, 16)])
def test_sizes_and_lane_splits_match_oracle(built, w, h, spp):
    """Ragged frames (partial blocks) and spp 1 / 3 / 5 / 16: split 1, uneven lanes per slot, split > 1."""
    for streaming in (False, True):
        sd = scenes.cbox(w, h)
        _exercised(*_exact(sd, seed=w + spp, spp=spp, streaming=streaming, seed_variant=spp % 2))


def test_wide_frame_medium_matches_oracle(built):
    """A frame wider than tall: Camera::importance refuses points with p.x > image_rect_max.y (sic, camera.rs:131), a band of columns on one
    side.  Only something inside that band can tell the quirk from `p.y > image_rect_max.y`: in the Cornell box the medium is."""
    sd = _with_back_triangle(scenes.cbox_medium(33, 17, 0.5, g=0.6))
    for streaming in (False, True):
        img, st = _exact(sd, seed=15, spp=3, streaming=streaming)
        _exercised(img, st)


def test_large_frame_split_one_matches_oracle(built):
    """rl_render_light keeps split = 1 while n_items >= CUs * kLightWaves * 4 * 64 * 2 = 524 288 on the MI355X's 256 CUs: 1024 x 512 at spp 2."""
    sd = scenes.cbox(1024, 512)
    _exercised(*_exact(sd, seed=9, spp=2))


def test_invalid_splats_match_oracle(built):
    """Coarse spheres (3 x 3 facets) with interpolated shading normals: near their silhouettes the shading-frame cosines of the light and of the
    camera direction disagree in sign with the geometric ones, so the unsigned `correction` (light.rs:107-108) goes negative and the splat is
    dropped as invalid (Color::is_valid)."""
    img, st = _exact(scenes.living_room(32, 24, n_spheres=27, tess=3), seed=10, spp=3)
    _exercised(img, st, "splats_invalid")


def _bright(sd, scale):
    for m in sd.meshes:
        if m.emission is not None:
            m.emission = tuple(float(c) * scale for c in m.emission)
    return sd


def _quantisation_bound(img, f64, counts, spp):
    """Every splat channel is rounded to 2^-24 (error <= 2^-25), the sum is exact, the resolve rounds once to f32: per pixel
    |image - f64 sum / spp| <= n_splats(pixel) * 2^-25 / spp + ulp(image) / 2 (+ the f64 sum's own rounding, far below)."""
    ok = np.isfinite(img)
    assert ok.all()
    assert (img >= 0.0).all()
    bound = counts[..., None].astype(np.float64) * 2.0 ** -25 / spp + np.abs(f64) * 2.0 ** -24 + 1e-300
    err = np.abs(img.astype(np.float64) - f64)
    assert (err <= bound * (1 + 1e-9)).all(), float((err / bound).max())


def test_saturated_splats_match_oracle(built):
    sd = _bright(scenes.cbox(16, 16), 1e12)
    img, st, f64, counts = _exact(sd, seed=11, spp=2, want_f64=True)
    _exercised(img, st, "splats_saturated")
    _quantisation_bound(img, f64, counts, 2)


def test_overflow_clamped_splats(built):
    """Clamped splats (2^31 = 2^55 in fixed point) pile up past 2^63 in a pixel of an 8 x 8 frame: the image must stay the true sum."""
    sd = _bright(scenes.cbox(8, 8), 1e13)
    spp = 64
    img, st, f64, counts = _exact(sd, seed=12, spp=spp, want_f64=True)
    _exercised(img, st, "splats_saturated")
    assert (f64 * spp).max() > 2.0 ** 39 * 2.0, (f64 * spp).max()          # past the old signed 64-bit limit, twice over
    _quantisation_bound(img, f64, counts, spp)


def test_overflow_bright_unclamped_splats(built):
    """Splats below the clamp whose sum in one pixel passes 2^39 (the old signed limit)."""
    sd = _bright(scenes.cbox(8, 8), 1e9)
    spp = 1024
    img, st, f64, counts = _exact(sd, seed=13, spp=spp, want_f64=True)
    _exercised(img, st)
    assert st["splats_saturated"] == 0
    assert (f64 * spp).max() > 2.0 ** 39 * 2.0, (f64 * spp).max()
    _quantisation_bound(img, f64, counts, spp)


def test_dim_light_quantisation(built):
    """Emission ~1e-6 (the Cornell light times 1e-6): a pixel's splats add up to a few 2^-24 steps.  The image keeps to the f64 sums within
    n_splats * 2^-25 / spp per pixel."""
    sd = _bright(scenes.cbox(24, 24), 1e-6)
    spp = 4
    img, st, f64, counts = _exact(sd, seed=14, spp=spp, want_f64=True)
    _exercised(img, st)
    assert (img > 0).mean() > 0.3 and np.median(f64[f64 > 0] * spp * 2.0 ** 24) < 16
    _quantisation_bound(img, f64, counts, spp)


def test_randomized_light_and_stratified_parity(built):
    """Short runs of the differential fuzzer's light-tracer and stratified arms (tests/parity_fuzz.py): its random scenes (no environment
    emitters for the light tracer), options, scene placements and, for the stratified sampler, pipelines, lanes and pool sizes."""
    from tests.parity_fuzz import run
    n, bad = run(budget=15.0, seed=11, arm="light")
    assert bad == 0 and n >= 20, (n, bad)
    n, bad = run(budget=15.0, seed=12, arm="stratified")
    assert bad == 0 and n >= 20, (n, bad)
