"""The edges of the camera-beam gather (kernels/gather.hip.h: beam_gather over BreLeaf / PlaneLeaf) that the fixtures of tests/test_gpu_bre_exact.py and
tests/test_gpu_plane_single_exact.py leave out, each held bit for bit to the restatements through the shared helpers of tests/gather_exact.py: media whose
three channels differ (a swapped or broadcast channel shows), a scattering coefficient with a zero channel (black for the photons, NaN in that channel and no
other for the plane strategies that divide by it), frames and blocks of a single row or column (the lane-to-pixel map), camera rays that leave the box and
still gather, a lane whose walk counters pass 2^24 (the high statistics rows of gather_split24 / gather_merge24), and three shards.  One process, no child."""
import functools
import json
import os

import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import bre_restatement as B
from tests import plane_single_restatement as P
from tests.gather_exact import BRE_KEYS, PLANE_KEYS, bre_exact, plane_exact
from tests.scene_helpers import context as _context

pytestmark = pytest.mark.gpu

SIGMA_A = (0.05, 0.3, 0.0)
SIGMA_S = (0.9, 0.4, 1.3)
SIGMA_S_ZERO = (0.9, 0.0, 1.3)
FRAMES = [(1, 1), (1, 17), (17, 1), (16, 16), (33, 16), (2, 35)]
FRAMES_AND_VARIANTS = [(w, h, 0) for w, h in FRAMES] + [(1, 17, 1), (17, 1, 1)]
HIGH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gather_high_counter.json")


def coloured(w, h, g=None, sigma_s=SIGMA_S):
    sd = scenes.cbox_medium(w, h, 1.0)
    sd.medium = scenes.Medium(SIGMA_A, sigma_s, scenes.PHASE_ISOTROPIC if g is None else scenes.PHASE_HG, 0.0 if g is None else g)
    return sd


# the restatement's results, computed once per process and shared by the LDS-staged and the streamed case; not to be modified
@functools.lru_cache(maxsize=None)
def _bre_ref(w, h, g, sigma_s, nb, spp, radius, seed=3, variant=0):
    return B.compute(coloured(w, h, g, sigma_s) if sigma_s else scenes.cbox_medium(w, h, 1.0), seed, nb, spp, None, 0, radius, variant)


@functools.lru_cache(maxsize=None)
def _plane_ref(w, h, sigma_s, strategy, nb, spp, seed=3, variant=0):
    return P.compute(coloured(w, h, None, sigma_s) if sigma_s else scenes.cbox_medium(w, h, 1.0), seed, nb, strategy, spp, variant)


def _channel_means_differ(img):
    m = [float(np.mean(img[..., k], dtype=np.float64)) for k in range(3)]
    assert np.isfinite(img).all() and m[0] != m[1] and m[1] != m[2] and m[0] != m[2] and min(m) > 0.0, m


# ---- coloured media
@pytest.mark.parametrize("streaming", [False, True])
@pytest.mark.parametrize("g", [None, -0.4])
def test_bre_coloured_medium(built, g, streaming):
    ref = _bre_ref(40, 24, g, SIGMA_S, 300, 3, 0.2)
    _channel_means_differ(ref["image"])
    _, st, _ = bre_exact(coloured(40, 24, g), nb_primitive=300, spp=3, radius=0.2, streaming=streaming, ref=ref)
    assert st["photons_gathered"] > 0


@pytest.mark.parametrize("streaming", [False, True])
@pytest.mark.parametrize("strategy", P.STRATEGIES)
def test_plane_coloured_medium(built, strategy, streaming):
    ref = _plane_ref(40, 24, SIGMA_S, strategy, 64, 2)
    _channel_means_differ(ref["image"])
    _, st, _ = plane_exact(coloured(40, 24), strategy, 64, spp=2, streaming=streaming, ref=ref)
    assert st["planes_visible"] > 0


# ---- sigma_s with a zero channel
def test_bre_zero_scattering_channel(built):
    """The photons carry no green; nothing divides by sigma_s."""
    ref = _bre_ref(24, 16, None, SIGMA_S_ZERO, 100, 2, 0.2)
    assert np.isfinite(ref["image"]).all() and not ref["image"][..., 1].any() and ref["image"][..., 0].any() and ref["image"][..., 2].any()
    bre_exact(coloured(24, 16, None, SIGMA_S_ZERO), nb_primitive=100, spp=2, radius=0.2, ref=ref)


@pytest.mark.parametrize("strategy", ["uv", "average", "discrete_mis"])
def test_plane_zero_scattering_channel(built, strategy):
    """The UV plane's weight is (PI * emission) / sigma_s, an unguarded Color / Color (plane_single.rs:195): inf in green, and inf * 0 = NaN once the gather
    multiplies by sigma_s again.  The device stores the same records and renders NaN in the same pixels of the same channel."""
    ref = _plane_ref(24, 16, SIGMA_S_ZERO, strategy, 64, 2)
    weights = ref["records"][:, 11:14].view(np.float32)
    assert not np.isfinite(weights[:, 1]).all() and np.isfinite(weights[:, [0, 2]]).all()
    img = ref["image"]
    assert np.isnan(img[..., 1]).any() and np.isfinite(img[..., [0, 2]]).all() and img[..., 0].any()
    got, _, _ = plane_exact(coloured(24, 16, None, SIGMA_S_ZERO), strategy, 64, spp=2, ref=ref)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(img))


# ---- the lane-to-pixel map: frames and blocks with a single row or column
@pytest.mark.parametrize("w,h,variant", FRAMES_AND_VARIANTS)
def test_bre_lane_map(built, w, h, variant):
    ref = _bre_ref(w, h, None, None, 120, 3, 0.3, 3, variant)
    bre_exact(scenes.cbox_medium(w, h, 1.0), nb_primitive=120, spp=3, radius=0.3, seed_variant=variant, ref=ref)


@pytest.mark.parametrize("w,h,variant", FRAMES_AND_VARIANTS)
def test_plane_lane_map(built, w, h, variant):
    ref = _plane_ref(w, h, None, "average", 33, 3, 3, variant)
    plane_exact(scenes.cbox_medium(w, h, 1.0), "average", 33, spp=3, seed_variant=variant, ref=ref)


# ---- camera rays that leave the box still gather (ray.tfar = f32::MAX)
def _missing_samples_that_gather(ref):
    miss = ref["detail"]["tfar"] == B.F32_MAX
    return int(np.count_nonzero(miss)), int(np.count_nonzero(ref["detail"]["c"][miss].any(axis=-1)))


def test_bre_camera_rays_that_miss(built):
    ref = _bre_ref(40, 24, None, SIGMA_S, 300, 3, 0.2)
    n_miss, n_gather = _missing_samples_that_gather(ref)
    assert n_miss > 0 and n_gather > 0, (n_miss, n_gather)
    bre_exact(coloured(40, 24), nb_primitive=300, spp=3, radius=0.2, ref=ref)


def test_plane_camera_rays_that_miss(built):
    ref = _plane_ref(40, 24, SIGMA_S, "average", 64, 2)
    n_miss, n_gather = _missing_samples_that_gather(ref)
    assert n_miss > 0 and n_gather > 0, (n_miss, n_gather)
    plane_exact(coloured(40, 24), "average", 64, spp=2, ref=ref)


# ---- a counter past 2^24 in one lane
def test_bre_counters_past_2_24_in_one_lane(built):
    """A 1x1 frame: the only lane walks every sample, and at the fixture's spp (the smallest multiple of 1024 that does it) both of its walk counters have
    passed 2^24, so their high parts travel through the rows of STAT_VERTICES / STAT_SHADOW_RAYS and gather_merge24 joins them.  The expected pixel and counters
    are the restatement's, stored by tests/golden/make_gather_high_counter.py (about 18 s on the CPU); the generation and the tree are held to the restatement
    here, at 1 spp.  Measured on an MI355X: the gather kernel takes 14.8 s (the test 15.0 s).  The time is the lane's 1.7e7 node visits and 1.9e7 gathered
    photons (three exact expf each) one after the other, about 0.4 us per element; 2^24 of each is the least that reaches the high rows, so more photons
    per sample at fewer samples leave the element count, and the time, where they are (measured: 8192 photons at 5632 spp, 14.3 s)."""
    with open(HIGH) as f:
        want = json.load(f)
    case, spp = want["case"], want["spp"]
    assert spp % 1024 == 0 and spp <= (1 << 22)                                   # RL_VPL_MAX_SPP
    assert want["stats"]["nodes_entered"] >= 1 << 24 and want["stats"]["photons_gathered"] >= 1 << 24
    assert want["below"]["spp"] == spp - 1024 and min(want["below"]["nodes_entered"], want["below"]["photons_gathered"]) < 1 << 24
    sd = scenes.cbox_medium(case["width"], case["height"], case["sigma_s"])
    _, _, ref = bre_exact(sd, seed=case["seed"], nb_primitive=case["nb_primitive"], spp=1, radius=case["radius"])
    assert (ref["records"].shape[0], ref["n_paths"]) == (want["records"], want["n_paths"])
    ctx = _context(sd)
    sampler = api.IndependentSampler(case["seed"])
    vpls, _ = ctx.vpl_generate(sampler, case["nb_primitive"], option_vpl=api.VPL_VOLUME)
    photons = ctx.photon_map(vpls, case["radius"])
    img, st = ctx.render_bre(photons, sampler.block_seeds(1, 1), spp)
    print("gather kernel ms:", st["ms_other"])
    for k in BRE_KEYS:
        print(k, st[k], want["stats"][k])
    for k in BRE_KEYS:
        assert st[k] == want["stats"][k], (k, st[k], want["stats"][k])
    np.testing.assert_array_equal(img.reshape(3).view(np.uint32), np.asarray(want["pixel_bits"], np.uint32))


# ---- three shards
def _three_shards(render, restate, keys):
    whole, st = render(0, 1)
    parts = [render(k, 3) for k in range(3)]
    assert whole.any()
    np.testing.assert_array_equal(parts[0][0] + parts[1][0] + parts[2][0], whole)
    lit = sum(p[0].any(axis=-1).astype(np.int32) for p in parts)
    assert lit.max() == 1
    for key in keys:
        assert sum(p[1][key] for p in parts) == st[key], key
    for k in range(3):                                # each shard against the restatement of that shard
        ref_img, ref_st = restate(k)
        np.testing.assert_array_equal(parts[k][0], ref_img)
        for key in keys:
            assert parts[k][1][key] == ref_st[key], (k, key)


def test_bre_three_shards_sum_to_the_frame(built):
    sd = scenes.cbox_medium(40, 40, 1.0)
    ctx = _context(sd)
    sampler = api.IndependentSampler(4)
    vpls, _ = ctx.vpl_generate(sampler, 200, option_vpl=api.VPL_VOLUME)
    photons = ctx.photon_map(vpls, 0.2)
    seeds = sampler.block_seeds(sd.width, sd.height)
    sc, words, n_paths = orc.Scene(sd), vpls.words(), vpls.info()[1]
    _three_shards(lambda k, n: ctx.render_bre(photons, seeds, 2, shard_index=k, shard_count=n),
                  lambda k: B.render(sc, sd, words, n_paths, seeds, 2, 0.2, 0, k, 3)[:2], BRE_KEYS)


def test_plane_three_shards_sum_to_the_frame(built):
    sd = scenes.cbox_medium(40, 40, 1.0)
    ctx = _context(sd)
    sampler = api.IndependentSampler(4)
    pset, _ = ctx.plane_generate(sampler, 64, "discrete_mis")
    pmap = ctx.plane_map(pset)
    seeds = sampler.block_seeds(sd.width, sd.height)
    sc, words, n_gen = orc.Scene(sd), pset.words(), pset.info()[1]
    _three_shards(lambda k, n: ctx.render_plane_single(pmap, seeds, 2, shard_index=k, shard_count=n),
                  lambda k: P.render(sc, sd, words, n_gen, "discrete_mis", seeds, 2, 0, k, 3)[:2], PLANE_KEYS)
