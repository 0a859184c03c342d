"""The virtual ray lights (rl_vrl_map_build / rl_render_vrl, kernels/vrl.hip.h) held bit for bit to the numpy restatement of the reference's text
(tests/vrl_restatement.py): the image (assert_array_equal) and every counter — the walked draws among them —, over LDS-staged and streamed BVHs, both stream
modes of the beam pass, grey, coloured, zero-scattering-channel and Henyey-Greenstein media, ragged and one-pixel-wide frames, spp 1 and 3, three shards, sets
with no VRL, one VRL and about 100, and hand-made records: bright VRLs among black ones (rr = 1), a tenth bright (rr about 0.1: the queues fill and drain), a
VRL behind the boxes, one of length 0, one through the camera position, and camera rays that miss the scene.  The map is read back against the partition,
avg and rr of the restatement; the refused inputs return their codes; the integrator class and the CLI give the bytes of the step-by-step sequence.  One
process; only the CLI test starts a child."""
import os
import subprocess

import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import cli
from tests import beam_restatement as R
from tests import vrl_restatement as V
from tests.beam_half_cases import assert_beam_half
from tests.scene_helpers import context as _context
from tests.test_gpu_gather_edges import SIGMA_S_ZERO, coloured

pytestmark = pytest.mark.gpu

RL_ERR_INVALID_ARGUMENT = -1


def _check_map(vmap, words, n_paths, radius):
    """The map read back: the host-only split and tree over the surface beams, the VRLs in storing order with the restatement's rr, avg."""
    surface, vrl_words = V.partition(words)
    got = vmap.read()
    n_sub, n_nodes = assert_beam_half(got, surface, radius)
    avg, rr = V.roulette(vrl_words)
    f = vrl_words.view(np.float32)
    want = np.zeros((vrl_words.shape[0], 12), np.float32)
    want[:, 0:4], want[:, 4:7], want[:, 7], want[:, 8:11] = f[:, 0:4], f[:, 4:7], rr, f[:, 8:11]
    np.testing.assert_array_equal(got[3].view(np.uint32), want.view(np.uint32))
    info = vmap.info()
    assert info[:5] == (surface.shape[0], n_sub, n_nodes, vrl_words.shape[0], n_paths) and info[5] == pytest.approx(radius)
    assert np.float32(info[6]) == avg
    return vrl_words.shape[0]


def _render_both(sd, ctx, sc, words, n_paths, vmap, seeds, spp, radius, variant=0, shard=(0, 1)):
    img, st = ctx.render_vrl(vmap, seeds, spp, variant, *shard)
    ref_img, ref_st, detail = V.render(sc, sd, words, n_paths, seeds, spp, radius, variant, *shard)
    for k in V.KEYS:
        assert st[k] == ref_st[k], (k, st[k], ref_st[k])
    np.testing.assert_array_equal(img, ref_img)
    return img, st, detail


def _exact(sd, seed=3, nb=60, spp=3, radius=0.1, max_depth=None, rr_depth=0, variant=0, streaming=False, streams="reference", need_visible=True):
    """Beam pass, map, chain pass and gather of one scene: the map against the restatement's partition, image and counters against the restatement."""
    ctx, sc = _context(sd, streaming), orc.Scene(sd)
    sampler = api.IndependentSampler(seed, variant)
    beams, _ = ctx.beam_generate(sampler, nb, max_depth, rr_depth, streams)
    words, (_, n_paths) = beams.words(), beams.info()
    vmap = ctx.vrl_map(beams, radius)
    n_vrl = _check_map(vmap, words, n_paths, radius)
    seeds = sampler.block_seeds(sd.width, sd.height)
    img, st, detail = _render_both(sd, ctx, sc, words, n_paths, vmap, seeds, spp, radius, variant)
    assert img.any()                                                # no case passes empty
    if n_vrl:
        assert st["vrl_accepted"] > 0
    if n_vrl and need_visible:
        assert st["vrl_visible"] > 0
        assert np.abs(detail["c"] - detail["c_beams"]).max() > 0    # and the VRLs reach the image
    return img, st, detail, n_vrl


@pytest.mark.parametrize("streaming", [False, True])
@pytest.mark.parametrize("streams", ["reference", "per_path"])
def test_grey_medium(built, streaming, streams):
    _, _, detail, n_vrl = _exact(scenes.cbox_medium(40, 24, 1.0), streaming=streaming, streams=streams)
    assert n_vrl > 0 and (detail["tfar"] == R.F32_MAX).any()        # camera rays that miss the scene take their draws all the same


@pytest.mark.parametrize("streaming", [False, True])
def test_coloured_medium(built, streaming):
    img, _, _, _ = _exact(coloured(40, 24), streaming=streaming)
    m = [float(np.mean(img[..., k], dtype=np.float64)) for k in range(3)]
    assert m[0] != m[1] and m[1] != m[2] and m[0] != m[2] and min(m) > 0.0, m


def test_zero_scattering_channel(built):
    img, _, _, _ = _exact(coloured(24, 16, None, SIGMA_S_ZERO), nb=50, spp=2)
    assert np.isfinite(img).all() and not img[..., 1].any() and img[..., 0].any() and img[..., 2].any()


def test_henyey_greenstein_medium_gathers_isotropically(built):
    """A beam's phase function is Isotropic whatever the medium's is (vol_primitives.rs:457, 483, 500): the restatement has no other."""
    _exact(scenes.cbox_medium(40, 24, 1.0, g=0.6), streaming=False)
    _exact(coloured(24, 16, g=-0.4), nb=50, spp=1, streaming=True)


@pytest.mark.parametrize("w,h,spp", [(40, 24, 1), (24, 16, 3), (1, 33, 3), (33, 1, 3), (1, 33, 1), (33, 1, 1)])
def test_frames_and_spp(built, w, h, spp):
    # (33 samples of a one-pixel-wide frame at spp 1 accept few of rr = 0.01 VRLs: more beams there, so that no case passes empty)
    # the 33 rays of the one-row frame at spp 1 pass the roulette 96 times and no pair is visible (most of the row looks past the box): the image there is the
    # surface beams', held bit for bit all the same
    _exact(scenes.cbox_medium(w, h, 1.0), nb=300 if w * h * spp < 40 else 40, spp=spp, radius=0.3, variant=1 if w == 1 else 0, need_visible=(w, h, spp) != (33, 1, 1))


def test_no_vrl(built):
    """max_depth = 2: the light's beam alone, no VRL; the image is the surface beams' and every sample takes two draws."""
    _, st, _, n_vrl = _exact(scenes.cbox_medium(24, 16, 1.0), seed=6, nb=1, spp=2, radius=0.5, max_depth=2)
    assert n_vrl == 0 and st["rng_draws"] == 2 * st["camera_samples"] and st["vrl_accepted"] == 0


def test_one_vrl(built):
    """The first seed and count whose set holds exactly one beam that leaves a volume vertex: rr = ((m / m) * 0.01).min(1.0) = 0.01."""
    sd = scenes.cbox_medium(24, 16, 1.0)
    ctx = _context(sd)
    for seed in range(40):
        for nb in (2, 3):
            beams, _ = ctx.beam_generate(api.IndependentSampler(seed), nb, 3)
            if int(((beams.words()[:, 7] & 1) == 0).sum()) == 1:
                _, st, _, n_vrl = _exact(sd, seed=seed, nb=nb, spp=3, radius=0.3, max_depth=3)
                assert n_vrl == 1
                return
    raise AssertionError("no seed below 40 gives a set with one VRL")


def test_about_100_vrls_and_depth_options(built):
    _, _, _, n_vrl = _exact(scenes.cbox_medium(24, 16, 1.0), seed=2, nb=200, spp=1, radius=0.05)
    assert 60 <= n_vrl <= 160, n_vrl
    _exact(scenes.cbox_medium(24, 16, 1.0), seed=2, nb=100, spp=2, max_depth=3, rr_depth=2, radius=0.2)


def test_three_shards_sum_to_the_frame(built):
    sd = scenes.cbox_medium(40, 40, 1.0)
    ctx, sc = _context(sd), orc.Scene(sd)
    sampler = api.IndependentSampler(4)
    beams, _ = ctx.beam_generate(sampler, 50)
    vmap = ctx.vrl_map(beams, 0.1)
    seeds = sampler.block_seeds(sd.width, sd.height)
    whole, st = ctx.render_vrl(vmap, seeds, 2)
    words, n_paths = beams.words(), beams.info()[1]
    parts = [_render_both(sd, ctx, sc, words, n_paths, vmap, seeds, 2, 0.1, 0, (k, 3)) for k in range(3)]
    assert whole.any() and st["vrl_accepted"] > 0
    np.testing.assert_array_equal(parts[0][0] + parts[1][0] + parts[2][0], whole)
    for k in V.KEYS:
        assert sum(p[1][k] for p in parts) == st[k], k


# ---- hand-made records through rl_vrl_map_build_words
def _surface(n=3, seed=5):
    rs = np.random.RandomState(seed)
    o = rs.uniform((-0.9, 0.1, -0.9), (0.9, 1.9, 0.9), (n, 3)).astype(np.float32)
    d = rs.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return R.beam_words(o, rs.uniform(0.3, 1.0, n).astype(np.float32), d, rs.uniform(0.5, 2.0, (n, 3)), from_surface=True)


def _cloud(n, seed, radiance):
    rs = np.random.RandomState(seed)
    o = rs.uniform((-0.8, 0.2, -0.8), (0.8, 1.8, 0.8), (n, 3)).astype(np.float32)
    d = rs.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return R.beam_words(o, rs.uniform(0.1, 0.6, n).astype(np.float32), d, radiance, from_surface=False, path=np.arange(n) % 5)


def _hand(sd, words, n_paths=5, spp=2, streaming=False, seed=8, radius=0.1):
    ctx, sc = _context(sd, streaming), orc.Scene(sd)
    vmap = ctx.vrl_map_from_words(words, n_paths, radius)
    _check_map(vmap, words, n_paths, radius)
    seeds = api.IndependentSampler(seed).block_seeds(sd.width, sd.height)
    img, st, detail = _render_both(sd, ctx, sc, words, n_paths, vmap, seeds, spp, radius)
    assert st["vrl_accepted"] > 0 and img.any()
    return img, st, detail


@pytest.mark.parametrize("streaming", [False, True])
def test_bright_vrls_among_black_ones(built, streaming):
    """Four bright VRLs among 400 black ones: avg is a hundredth of the bright ones' radiance, so rr = 1 for them and 0 for the rest."""
    rad = np.zeros((404, 3), np.float32)
    rad[[7, 150, 151, 399]] = (3.0, 2.0, 1.0)
    words = np.concatenate([_surface(), _cloud(404, 21, rad)])
    _, st, detail = _hand(scenes.cbox_medium(24, 16, 1.0), words, spp=1, streaming=streaming)
    rr = detail["vrls"].rr
    assert (rr[[7, 150, 151, 399]] == 1.0).all() and np.count_nonzero(rr) == 4
    assert st["vrl_accepted"] >= 4 * st["camera_samples"]


@pytest.mark.parametrize("streaming", [False, True])
def test_a_tenth_bright(built, streaming):
    """40 bright VRLs among 400: rr is about 0.1 for them; lanes accept a few each and at different VRLs, so queues fill, trigger and drain."""
    rad = np.zeros((400, 3), np.float32)
    rad[::10] = (2.0, 2.0, 2.0)
    words = np.concatenate([_surface(), _cloud(400, 22, rad)])
    _, st, detail = _hand(scenes.cbox_medium(40, 24, 1.0), words, spp=2, streaming=streaming)
    rr = detail["vrls"].rr
    assert np.allclose(rr[::10], 0.1) and st["vrl_accepted"] > 2 * st["camera_samples"]
    per_sample = np.bincount(detail["entries"][0], minlength=detail["d"].shape[0])
    assert per_sample.max() >= 5                                      # more than a queue holds


def test_special_vrls(built):
    """A VRL behind the boxes (some of its pairs are occluded), one of length 0 (inv_pdf = 0), one through the camera position, one in the open, and a frame
    whose edge rays miss the scene.  400 black VRLs bring avg down, so the four bright ones have rr = 1 and every sample evaluates them."""
    sd = scenes.cbox_medium(40, 24, 1.0)
    sc = orc.Scene(sd)
    cam, _ = sc.camera_generate(sd.width / 2, sd.height / 2)
    cam = np.asarray(cam, np.float32)
    x = np.asarray([1.0, 0.0, 0.0], np.float32)
    bright = (300.0, 200.0, 100.0)
    vr = np.concatenate([
        R.beam_words([(-0.9, 0.3, -0.75)], 1.0, [x], [bright], from_surface=False),               # behind the boxes, low
        R.beam_words([(0.3, 0.7, 0.2)], 0.0, [(0.0, 1.0, 0.0)], [bright], from_surface=False),    # length 0
        R.beam_words([cam - x * np.float32(0.5)], 1.0, [x], [bright], from_surface=False),        # through the camera position
        R.beam_words([(0.0, 1.0, 0.0)], 0.5, [(0.0, 1.0, 0.0)], [bright], from_surface=False),
    ])
    words = np.concatenate([_surface(), vr, _cloud(400, 23, np.zeros((400, 3), np.float32))])
    _, st, detail = _hand(sd, words, spp=2)
    assert (detail["vrls"].rr[:4] == 1.0).all()
    assert 0 < st["vrl_visible"] < st["vrl_accepted"]
    e_s, e_v = detail["entries"][0], detail["entries"][1]
    assert np.isfinite(detail["val"]).all()
    assert not detail["val"][e_v == 1].any()                          # length 0: inv_pdf = 0
    miss = detail["tfar"][e_s] == R.F32_MAX
    assert miss.any() and not detail["val"][miss].any()               # a miss takes its draws and contributes zero
    occluded = (e_v == 0) & ~detail["visible"]
    assert occluded.any() and ((e_v == 0) & detail["visible"]).any()


def test_refused_inputs(built):
    plain = _context(scenes.cbox(16, 16))                             # no medium
    words = np.concatenate([_surface(), _cloud(3, 1, (1.0, 1.0, 1.0))])
    with pytest.raises(api.RustlightError) as e:
        plain.vrl_map_from_words(words, 1, 0.1)
    assert e.value.code == api.RL_ERR_UNSUPPORTED
    sd = scenes.cbox_medium(16, 16, 1.0)
    ctx, other = _context(sd), _context(sd)
    s = api.IndependentSampler(0)
    beams, _ = ctx.beam_generate(s, 16)
    for radius in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(api.RustlightError) as e:
            ctx.vrl_map(beams, radius)
        assert e.value.code == RL_ERR_INVALID_ARGUMENT, radius
    with pytest.raises(api.RustlightError) as e:
        other.vrl_map(beams, 0.2)                                     # a set from another context
    assert e.value.code == RL_ERR_INVALID_ARGUMENT
    with pytest.raises(api.RustlightError) as e:
        ctx.vrl_map_from_words(words, 0, 0.1)                         # no light path to normalise by
    assert e.value.code == RL_ERR_INVALID_ARGUMENT
    with pytest.raises(api.RustlightError) as e:
        ctx.vrl_map_from_words(_cloud(3, 1, (1.0, 1.0, 1.0)), 1, 0.1)     # no surface beam
    assert e.value.code == RL_ERR_INVALID_ARGUMENT and "surface" in str(e.value)
    for word in (1, 3, 5, 9):                                         # o, length, d, radiance of a VRL record
        bad = words.copy()
        bad[4, word] = np.float32("inf" if word == 9 else "nan").view(np.uint32)
        with pytest.raises(api.RustlightError) as e:
            ctx.vrl_map_from_words(bad, 1, 0.1)
        assert e.value.code == RL_ERR_INVALID_ARGUMENT, word
    bad = words.copy()
    bad[0, 5] = np.float32("nan").view(np.uint32)                     # a surface beam: what rl_beam_map_build_words refuses
    with pytest.raises(api.RustlightError) as e:
        ctx.vrl_map_from_words(bad, 1, 0.1)
    assert e.value.code == RL_ERR_INVALID_ARGUMENT
    vmap = ctx.vrl_map(beams, 0.2)
    seeds = s.block_seeds(16, 16)
    with pytest.raises(api.RustlightError) as e:
        other.render_vrl(vmap, seeds)                                 # a map from another context
    assert e.value.code == RL_ERR_INVALID_ARGUMENT
    for kw, code in (({"spp": (1 << 22) + 1}, api.RL_ERR_UNSUPPORTED), ({"spp": 0}, RL_ERR_INVALID_ARGUMENT),
                     ({"shard_index": 2, "shard_count": 2}, RL_ERR_INVALID_ARGUMENT)):
        with pytest.raises(api.RustlightError) as e:
            ctx.render_vrl(vmap, seeds, **kw)
        assert e.value.code == code, kw
    # 256 * spp * (2 + 3 * n_vrl) >= 2^32: 4000 VRLs at spp 1400 (below RL_VPL_MAX_SPP)
    many = ctx.vrl_map_from_words(np.concatenate([_surface(), _cloud(4000, 2, (1.0, 1.0, 1.0))]), 1, 0.1)
    assert 256 * 1400 * (2 + 3 * 4000) >= 1 << 32 > 256 * 1397 * (2 + 3 * 4000)
    with pytest.raises(api.RustlightError) as e:
        ctx.render_vrl(many, seeds, spp=1400)
    assert e.value.code == api.RL_ERR_UNSUPPORTED and "spp = 1400" in str(e.value) and "VRLs = 4000" in str(e.value)


def test_integrator_compute(built):
    """IntegratorVirtualRayLights::compute is the sequence of _exact: generate, map, block seeds from the sampler the generation leaves, render."""
    sd = scenes.cbox_medium(24, 16, 1.0)
    for streams in api.LIGHT_STREAMS:
        integ = api.IntegratorVirtualRayLights(nb_primitive=60, radius=0.1, light_streams=streams)
        img = integ.compute(api.IndependentSampler(9), api.Scene(sd), 2)
        want, st, _, _ = _exact(sd, seed=9, nb=60, spp=2, radius=0.1, streams=streams)
        np.testing.assert_array_equal(img, want)
        assert integ.last_stats["vrl_accepted"] == st["vrl_accepted"] and integ.last_stats["rng_draws"] == st["rng_draws"]


def test_cli_renders_what_the_api_renders(built, tmp_path):
    """`virtual-ray-lights` goes through the C++ mirror (integrator.hpp: IntegratorVirtualRayLights::compute): the same bytes as the Python mirror."""
    scn = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "cbox.pbrt")
    out = str(tmp_path / "out.pfm")
    args = [cli.EXE, scn, "-n", "2", "-r", "independent:7", "-m", "1.0", "-o", out]
    for extra, streams in (([], "reference"), (["--light-streams", "per-path"], "per_path")):
        r = subprocess.run(args + ["virtual-ray-lights", "--nb-primitive", "100", "--radius", "0.1", "-m", "6", "-r", "3"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        img = api.load_pfm(out)
        scene = api.Scene.load(scn)
        scene.set_medium((0.0,) * 3, (1.0,) * 3)
        integ = api.IntegratorVirtualRayLights(nb_primitive=100, max_depth=6, rr_depth=3, radius=0.1, light_streams=streams)
        want = integ.compute(api.IndependentSampler(7), scene, 2)
        assert img.shape == want.shape and want.any() and integ.last_stats["vrl_accepted"] > 0
        np.testing.assert_array_equal(img, want)
