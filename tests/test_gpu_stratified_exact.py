"""RL_STREAM_STRATIFIED (kernels/sampler.hip.h) held to the CPU oracle's restatement of the sampler's specification (oracle/rl_oracle.cpp, namespace
strat): the raw draws bit for bit, then `path`, `ao` and `direct` images and counters bit for bit in every execution form.  A wrong dimension, a
drifting dimension counter between wavefront launches or a wrong pixel key shared by all GPU forms fails here.  One process, no child."""
import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes

pytestmark = pytest.mark.gpu

# six next() and six next2d() in a mixed order: past the fourth dimension of each kind the plain Rng draws
PATTERN = [1, 2, 1, 1, 2, 2, 1, 2, 1, 2, 1, 2]
PATH_KEYS = ("camera_samples", "vertices", "extension_rays", "shadow_rays", "rng_draws")


@pytest.mark.parametrize("spp", [1, 2, 3, 5, 16, 17, 64, 1000])
def test_draws_match_oracle(built, spp):
    rng = np.random.default_rng(77 + spp)
    seeds = rng.integers(0, 2 ** 63, size=300, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=300, dtype=np.uint64)
    for variant in (0, 1):
        got = api.stratified_draws(seeds, spp, PATTERN, seed_variant=variant)
        ref = orc.stratified_draws(seeds, spp, PATTERN, seed_variant=variant)
        np.testing.assert_array_equal(got, ref)
        assert got.shape == (300, spp, 18) and np.unique(got).size > 100


def _path_scene(which):
    if which == "cbox": return scenes.cbox(40, 32)
    if which == "mixed": return scenes.living_room(48, 32, n_spheres=27, tess=8)
    return scenes.cbox_medium(32, 32, 0.5, 0.1, g=0.6)


def _assert_path(got, ref):
    (img, st), (rimg, rst) = got, ref
    for k in PATH_KEYS:
        assert st[k] == rst[k], (k, st[k], rst[k])
    np.testing.assert_array_equal(img, rimg)
    assert img.mean() > 0


@pytest.mark.parametrize("which", ["cbox", "mixed", "medium"])
def test_path_matches_oracle_in_every_form(built, which):
    sd = _path_scene(which)
    spp = 5
    max_depth = 8 if which == "mixed" else None
    scene = api.Scene(sd)
    ctx, osc = api.Context(scene, 0), orc.Scene(sd)
    seeds = api.IndependentSampler(21).block_seeds(sd.width, sd.height)
    P = lambda **kw: api.path_params(spp=spp, stream_mode=api.STREAM_STRATIFIED, max_depth=max_depth, **kw)
    ref = osc.render(seeds=seeds, spp=spp, stream_mode=api.STREAM_STRATIFIED, max_depth=max_depth, eval_order=1)
    _assert_path(ctx.render(seeds, P(pipeline=api.PIPELINE_FUSED)), ref)
    _assert_path(ctx.render(seeds, P(pipeline=api.PIPELINE_WAVEFRONT)), ref)
    _assert_path(ctx.render(seeds, P(pipeline=api.PIPELINE_WAVEFRONT, pool_slots=1024)), ref)
    for split in (1, 3, 4):
        _assert_path(ctx.render(seeds, P(sample_split=split)), ref)
        _assert_path(ctx.render(seeds, P(pipeline=api.PIPELINE_WAVEFRONT, sample_split=split)), ref)
    for r in range(3):
        shard = osc.render(seeds=seeds, spp=spp, stream_mode=api.STREAM_STRATIFIED, max_depth=max_depth, eval_order=1, shard_index=r, shard_count=3)
        _assert_path(ctx.render(seeds, P(shard_index=r, shard_count=3)), shard)
    multi = api.MultiContext(scene, 2, devices=[0, 0])
    try:
        np.testing.assert_array_equal(multi.render(seeds, P())[0], ref[0])
    finally:
        multi.close()
    # the other seed variant and other depth options through the same sampler
    v1 = osc.render(seeds=api.IndependentSampler(22, 1).block_seeds(sd.width, sd.height), spp=3, stream_mode=api.STREAM_STRATIFIED, seed_variant=1,
                    min_depth=1, max_depth=5, rr_depth=1, eval_order=1)
    _assert_path(ctx.render(api.IndependentSampler(22, 1).block_seeds(sd.width, sd.height),
                            api.path_params(spp=3, stream_mode=api.STREAM_STRATIFIED, seed_variant=1, min_depth=1, max_depth=5, rr_depth=1)), v1)


def test_ao_and_direct_match_oracle(built):
    """The option sets of test_ao_and_direct_integrators_parity with the stratified sampler."""
    mode = api.STREAM_STRATIFIED
    for sd in (scenes.cbox(48, 40), scenes.cbox_other_lights(40, 40), scenes.sky_scene(40, 40, keep_area_light=True), scenes.living_room(48, 32, n_spheres=20, tess=8)):
        ctx, osc = api.Context(api.Scene(sd), 0), orc.Scene(sd)
        seeds = api.IndependentSampler(4).block_seeds(sd.width, sd.height)
        for kw in (dict(max_distance=1.0), dict(max_distance=None), dict(max_distance=0.3, normal_correction=True)):
            img, st = ctx.render_ao(seeds, spp=3, stream_mode=mode, **kw)
            ref, ost = osc.render_ao(seeds=seeds, spp=3, stream_mode=mode, **kw)
            np.testing.assert_array_equal(img, ref)
            assert all(st[k] == ost[k] for k in ("camera_samples", "extension_rays", "rng_draws"))
            assert img.mean() > 0
        for kw in (dict(), dict(nb_bsdf_samples=2, nb_light_samples=3), dict(nb_bsdf_samples=0, nb_light_samples=1), dict(nb_bsdf_samples=1, nb_light_samples=0)):
            img, st = ctx.render_direct(seeds, spp=3, stream_mode=mode, **kw)
            ref, ost = osc.render_direct(seeds=seeds, spp=3, stream_mode=mode, **kw)
            np.testing.assert_array_equal(img, ref)
            assert all(st[k] == ost[k] for k in ("camera_samples", "extension_rays", "shadow_rays", "rng_draws"))
            assert img.mean() > 0
