"""IntegratorVPL (rl_vpl_generate / rl_render_vpl, kernels/vpl.hip.h) held bit for bit to the CPU oracle's restatement (oracle/rl_oracle.cpp:
orc_vpl_generate, orc_render_vpl, written from src/integrators/explicit/vpl.rs): the VPL records, the path count and the advanced sampler, then the
image and every counter both sides report, over scenes that reach each instantiation (BSDF types, the medium, point / directional lights, uv
emission), every -l x -v combination with a medium, LDS-staged and streamed BVHs, a ragged frame, spp 1 and 5, both seed variants and two shards.
The refused inputs return their codes.  The randomized arm of tests/parity_fuzz.py ("vpl") runs from here.  One process, no child."""
import os

import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import cli
from tests.scene_helpers import context as _context, glass_and_mirror as _glass_and_mirror, single_bsdf as _single_bsdf, with_back_triangle as _with_back_triangle

pytestmark = pytest.mark.gpu

RL_ERR_INVALID_ARGUMENT = -1
GEN_KEYS = ("camera_samples", "vertices", "extension_rays", "rng_draws")
KEYS = ("camera_samples", "extension_rays", "shadow_rays", "rng_draws", "gather_surface", "gather_volume")


def _exact(sd, seed=0, nb_vpl=32, spp=1, max_depth=None, rr_depth=0, option_vpl=api.VPL_ALL, option_lt=api.VPL_ALL, seed_variant=0, streaming=False, ctx=None):
    """IntegratorVPL::compute on the GPU and in the restatement, step by step.  Returns (image, gather stats, generation stats)."""
    ctx = ctx or _context(sd, streaming)
    ref = orc.vpl_compute(sd, seed, nb_vpl, spp, max_depth, rr_depth, option_vpl, option_lt, seed_variant)
    sampler = api.IndependentSampler(seed, seed_variant)
    vpls, gst = ctx.vpl_generate(sampler, nb_vpl, max_depth, rr_depth, option_vpl)
    np.testing.assert_array_equal(vpls.words(), ref["records"])
    assert vpls.info() == (ref["records"].shape[0], ref["n_paths"]) and ref["records"].shape[0] >= nb_vpl
    assert list(sampler.s.s) == [int(v) for v in ref["state"]]
    for k in GEN_KEYS:
        assert gst[k] == ref["gen_stats"][k], (k, gst[k], ref["gen_stats"][k])
    seeds = sampler.block_seeds(sd.width, sd.height)
    np.testing.assert_array_equal(seeds, ref["seeds"])
    img, st = ctx.render_vpl(vpls, seeds, spp, option_lt, seed_variant)
    for k in KEYS:
        assert st[k] == ref["stats"][k], (k, st[k], ref["stats"][k])
    np.testing.assert_array_equal(img, ref["image"])
    assert st["camera_samples"] == spp * sd.width * sd.height
    assert st["rng_draws"] == (3 if sd.medium is not None else 2) * st["camera_samples"]
    return img, st, gst


def _scene(name, w=24, h=24):
    if name == "cbox": return scenes.cbox(w, h)
    if name == "medium": return _with_back_triangle(scenes.cbox_medium(w, h, 0.5, g=0.6))
    if name == "point": return scenes.cbox_other_lights(w, h, point=True, directional=False, environment=False, keep_area_light=True)
    if name == "directional": return scenes.cbox_other_lights(w, h, point=False, directional=True, environment=False, keep_area_light=True)
    if name == "hsv": return scenes.override_light_emission(scenes.cbox(w, h), "hsv")
    if name == "texture":
        sd = scenes.cbox(w, h)
        sd.bitmaps.append((4, 4, np.linspace(0.1, 2.0, 48, dtype=np.float32).reshape(4, 4, 3)))
        return scenes.override_light_emission(sd, "texture", bitmap_id=0)
    if name == "glass_and_mirror": return _glass_and_mirror(w, h)          # several BSDF types: the run-time switch; glass transmission carries eta^2 into the RR
    if name == "glass": return _single_bsdf(w, h, scenes.Bsdf(type=scenes.GLASS))
    if name == "phong": return _single_bsdf(w, h, scenes.living_room_materials()[1])
    if name == "rough_metal": return _single_bsdf(w, h, scenes.Bsdf(type=scenes.METAL, specular=scenes.const_color((0.9, 0.8, 0.7)), distribution=scenes.MF_GGX, alpha_u=0.3, alpha_v=0.3))
    if name == "substrate": return _single_bsdf(w, h, scenes.living_room_materials()[5])
    if name == "mixed": return scenes.living_room(w + 8, h, n_spheres=8, tess=6)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["cbox", "medium", "point", "directional", "hsv", "texture", "glass_and_mirror", "phong", "rough_metal", "substrate", "mixed"])
def test_scenes_match_restatement(built, name):
    img, st, gst = _exact(_scene(name), seed=3)
    assert img.any() and st["gather_surface"] > 0 and gst["camera_samples"] > 0
    if name == "medium":
        assert st["gather_volume"] > 0


def test_glass_only_scene_matches_restatement(built):
    """Every surface smooth: no surface VPL, no gather ray, only the emitter VPLs and self emission."""
    img, st, _ = _exact(_scene("glass"), seed=1, max_depth=6)
    assert st["shadow_rays"] == 0


@pytest.mark.parametrize("option_lt", [api.VPL_ALL, api.VPL_SURFACE, api.VPL_VOLUME])
@pytest.mark.parametrize("option_vpl", [api.VPL_ALL, api.VPL_SURFACE, api.VPL_VOLUME])
def test_medium_options_match_restatement(built, option_vpl, option_lt):
    _exact(_scene("medium", 20, 12), seed=5, nb_vpl=24, option_vpl=option_vpl, option_lt=option_lt)


@pytest.mark.parametrize("name", ["cbox", "medium"])
def test_streamed_bvh_matches_restatement(built, name):
    ctx = _context(_scene(name), streaming=True)
    assert ctx.scene is not None
    _exact(_scene(name), seed=7, ctx=ctx)


@pytest.mark.parametrize("spp,variant", [(1, 1), (5, 0), (5, 1)])
def test_ragged_frame_spp_and_seed_variants(built, spp, variant):
    _exact(scenes.cbox(40, 24), seed=11, spp=spp, seed_variant=variant, nb_vpl=20)


def test_depth_and_rr_options(built):
    _exact(_scene("cbox"), seed=2, max_depth=2)           # emitter VPLs only
    _exact(_scene("cbox"), seed=2, max_depth=4, rr_depth=None)
    _exact(_scene("medium", 16, 16), seed=2, max_depth=3, rr_depth=2)


def test_two_shards_sum_to_the_frame(built):
    sd = scenes.cbox(40, 40)
    ctx = _context(sd)
    sampler = api.IndependentSampler(4)
    vpls, _ = ctx.vpl_generate(sampler, 16)
    seeds = sampler.block_seeds(sd.width, sd.height)
    whole, st = ctx.render_vpl(vpls, seeds, 2)
    parts = [ctx.render_vpl(vpls, seeds, 2, shard_index=k, shard_count=2) for k in range(2)]
    np.testing.assert_array_equal(parts[0][0] + parts[1][0], whole)
    assert not np.logical_and(parts[0][0].any(axis=-1), parts[1][0].any(axis=-1)).any()
    for k in KEYS:
        assert parts[0][1][k] + parts[1][1][k] == st[k], k


def test_randomized_vpl_parity(built):
    """A short run of the differential fuzzer's vpl arm (tests/parity_fuzz.py): the fuzzer's scene kinds that the generation accepts, a coloured medium on a third of them, every
    -v x -l pair, depth options, streamed BVHs, a third of the sets from per-path streams under a random batch size, one shard of 2-4."""
    from tests.parity_fuzz import run
    n, bad = run(budget=15.0, seed=23, arm="vpl")
    assert bad == 0 and n >= 20, (n, bad)


def test_refused_inputs(built):
    sd = scenes.cbox(16, 16)
    ctx = _context(sd)
    s = api.IndependentSampler(0)
    before = list(s.s.s)
    for kw, code in (({"max_depth": 1}, RL_ERR_INVALID_ARGUMENT), ({"nb_vpl": 0}, RL_ERR_INVALID_ARGUMENT),
                     ({"option_vpl": 3}, RL_ERR_INVALID_ARGUMENT), ({"option_vpl": api.VPL_VOLUME}, api.RL_ERR_UNSUPPORTED)):
        with pytest.raises(api.RustlightError) as e:
            ctx.vpl_generate(s, **kw)
        assert e.value.code == code, kw
    assert list(s.s.s) == before                     # nothing ran
    vpls, _ = ctx.vpl_generate(s, 8)
    seeds = s.block_seeds(16, 16)
    for kw, code in (({"stream_mode": api.STREAM_PER_SAMPLE}, api.RL_ERR_UNSUPPORTED), ({"numerics": api.NUMERICS_FAST}, api.RL_ERR_UNSUPPORTED),
                     ({"option_lt": 3}, RL_ERR_INVALID_ARGUMENT), ({"spp": (1 << 22) + 1}, api.RL_ERR_UNSUPPORTED),
                     ({"shard_index": 2, "shard_count": 2}, RL_ERR_INVALID_ARGUMENT)):
        with pytest.raises(api.RustlightError) as e:
            ctx.render_vpl(vpls, seeds, **kw)
        assert e.value.code == code, kw
    other = _context(sd)
    with pytest.raises(api.RustlightError):
        other.render_vpl(vpls, seeds)                # a set from another context
    # a directional light with a medium (the reference asserts), and no emitter
    dm = _scene("medium", 8, 8)
    dm.lights.append({"type": "directional", "a": (0.0, -1.0, 0.0), "intensity": (1.0, 1.0, 1.0)})
    with pytest.raises(api.RustlightError) as e:
        _context(dm).vpl_generate(api.IndependentSampler(0), 8)
    assert e.value.code == api.RL_ERR_UNSUPPORTED
    dark = scenes.cbox(8, 8)
    dark.meshes = [m for m in dark.meshes if m.emission is None]
    with pytest.raises(api.RustlightError) as e:
        _context(dark).vpl_generate(api.IndependentSampler(0), 8)
    assert e.value.code == api.RL_ERR_NO_EMITTER


def test_integrator_compute_and_records(built):
    sd = scenes.cbox(24, 16)
    integ = api.IntegratorVPL(nb_vpl=40)
    img = integ.compute(api.IndependentSampler(9), api.Scene(sd), 2)
    ref = orc.vpl_compute(sd, 9, 40, 2)
    np.testing.assert_array_equal(img, ref["image"])
    ctx = _context(sd)
    vpls, _ = ctx.vpl_generate(api.IndependentSampler(9), 40)
    rec = vpls.records()
    assert rec.shape == (ref["records"].shape[0],) and set(np.unique(rec["kind"])) <= {0, 2}
    np.testing.assert_array_equal(rec["pos"].view(np.uint32), ref["records"][:, 4:7])


def test_cli_renders_what_the_api_renders(built, tmp_path):
    import subprocess
    scn = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "cbox.pbrt")
    out = str(tmp_path / "out.pfm")
    r = subprocess.run([cli.EXE, scn, "-n", "2", "-r", "independent:7", "-o", out, "vpl", "--nb-vpl", "48", "-b", "1.5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img = api.load_pfm(out)
    want = api.IntegratorVPL(nb_vpl=48).compute(api.IndependentSampler(7), api.Scene.load(scn), 2)
    assert img.shape == want.shape and want.any()
    np.testing.assert_array_equal(img, want)
