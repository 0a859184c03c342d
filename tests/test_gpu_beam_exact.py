"""The photon beams' gather (rl_beam_map_build / rl_render_beams, kernels/beam.hip.h) held bit for bit to the numpy restatement of the reference's text
(tests/beam_restatement.py): the image (assert_array_equal) and every counter, over LDS-staged and streamed BVHs, grey, coloured, zero-scattering-channel and
Henyey-Greenstein media, ragged and one-pixel-wide frames, spp 1 and 3, three shards, both stream modes of the beam pass, sets from one beam (5 or 6 sub-beams) to
about 2000 sub-beams, and hand-made beams.  The beams come from the device's own beam pass, which tests/test_gpu_beam_records.py holds to the oracle's light
paths.  The split of a non-empty set makes at least 5 sub-beams (tests/test_beam_restatement.py says why); trees of 1 to 4 sub-beams are compared there, on
the host.  The refused inputs return their codes; the CLI writes the bytes the API renders.  One process; only the CLI test starts a child."""
import os
import subprocess

import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import cli
from tests import beam_restatement as R
from tests.beam_half_cases import assert_beam_half
from tests.scene_helpers import context as _context
from tests.test_gpu_gather_edges import SIGMA_S_ZERO, coloured

pytestmark = pytest.mark.gpu

RL_ERR_INVALID_ARGUMENT = -1


def _render_both(sd, ctx, sc, words, n_paths, bmap, seeds, spp, radius, variant=0, shard=(0, 1)):
    img, st = ctx.render_beams(bmap, seeds, spp, variant, *shard)
    ref_img, ref_st, detail = R.render(sc, sd, words, n_paths, seeds, spp, radius, variant, *shard)
    np.testing.assert_array_equal(img, ref_img)
    for k in R.KEYS:
        assert st[k] == ref_st[k], k
    return img, st, detail


def _exact(sd, seed=3, nb=120, spp=3, radius=0.1, max_depth=None, rr_depth=0, variant=0, streaming=False, streams="reference"):
    """Beam pass, map and gather of one scene: the map against the host-only build, image and counters against the restatement."""
    ctx, sc = _context(sd, streaming), orc.Scene(sd)
    sampler = api.IndependentSampler(seed, variant)
    beams, _ = ctx.beam_generate(sampler, nb, max_depth, rr_depth, streams)
    words, (n_beams, n_paths) = beams.words(), beams.info()
    bmap = ctx.beam_map(beams, radius)
    n_sub, n_nodes = assert_beam_half(bmap.read(), words, radius)
    assert bmap.info() == (n_beams, n_sub, n_nodes, n_paths, pytest.approx(radius))
    seeds = sampler.block_seeds(sd.width, sd.height)
    img, st, detail = _render_both(sd, ctx, sc, words, n_paths, bmap, seeds, spp, radius, variant)
    assert st["beams_accepted"] > 0 and img.any()                 # no case passes empty
    return img, st, detail


@pytest.mark.parametrize("streaming", [False, True])
@pytest.mark.parametrize("streams", ["reference", "per_path"])
def test_grey_medium(built, streaming, streams):
    _, _, detail = _exact(scenes.cbox_medium(40, 24, 1.0), streaming=streaming, streams=streams)
    assert (detail["tfar"] == R.F32_MAX).any()                    # camera rays that miss the scene still gather


@pytest.mark.parametrize("streaming", [False, True])
def test_coloured_medium(built, streaming):
    img, _, _ = _exact(coloured(40, 24), streaming=streaming)
    m = [float(np.mean(img[..., k], dtype=np.float64)) for k in range(3)]
    assert m[0] != m[1] and m[1] != m[2] and m[0] != m[2] and min(m) > 0.0, m


def test_zero_scattering_channel(built):
    img, _, _ = _exact(coloured(24, 16, None, SIGMA_S_ZERO), nb=100, spp=2)
    assert np.isfinite(img).all() and not img[..., 1].any() and img[..., 0].any() and img[..., 2].any()


def test_henyey_greenstein_medium_gathers_isotropically(built):
    """The beams' phase function is Isotropic whatever the medium's is (vol_primitives.rs:457): the restatement has no other."""
    _exact(scenes.cbox_medium(40, 24, 1.0, g=0.6), streaming=False)
    _exact(coloured(24, 16, g=-0.4), nb=100, spp=1, streaming=True)


@pytest.mark.parametrize("w,h,spp", [(40, 24, 1), (1, 33, 3), (33, 1, 3), (1, 33, 1), (33, 1, 1)])
def test_frames_and_spp(built, w, h, spp):
    _exact(scenes.cbox_medium(w, h, 1.0), nb=80, spp=spp, radius=0.3, variant=1 if w == 1 else 0)


def test_about_2000_sub_beams_and_depth_options(built):
    _, _, detail = _exact(scenes.cbox_medium(24, 16, 1.0), seed=2, nb=400, spp=1, radius=0.05)
    assert 1900 <= detail["sub"].shape[0] <= 2500
    _exact(scenes.cbox_medium(24, 16, 1.0), seed=2, nb=100, spp=2, max_depth=3, rr_depth=2, radius=0.2)


def test_one_beam(built):
    """max_depth = 2 and nb_primitive = 1: one beam from the light, the fewest sub-beams a split makes (5, or 6 where length / (length / 5) rounds up past 5):
    the first inner node over two leaves; a radius a quarter of the box."""
    _, st, detail = _exact(scenes.cbox_medium(24, 16, 1.0), seed=6, nb=1, spp=2, radius=0.5, max_depth=2)
    assert detail["sub"].shape[0] in (5, 6) and len(detail["tree"]["nodes"]) == 3


def test_three_shards_sum_to_the_frame(built):
    sd = scenes.cbox_medium(40, 40, 1.0)
    ctx, sc = _context(sd), orc.Scene(sd)
    sampler = api.IndependentSampler(4)
    beams, _ = ctx.beam_generate(sampler, 100)
    bmap = ctx.beam_map(beams, 0.1)
    seeds = sampler.block_seeds(sd.width, sd.height)
    whole, st = ctx.render_beams(bmap, seeds, 2)
    words, n_paths = beams.words(), beams.info()[1]
    parts = [_render_both(sd, ctx, sc, words, n_paths, bmap, seeds, 2, 0.1, 0, (k, 3)) for k in range(3)]
    assert whole.any()
    np.testing.assert_array_equal(parts[0][0] + parts[1][0] + parts[2][0], whole)
    for k in R.KEYS:
        assert sum(p[1][k] for p in parts) == st[k], k


# ---- hand-made beams through rl_beam_map_build_words
def _hand_made(sd):
    """Beams in and beside the box: a cloud, then a beam parallel to the central camera ray, a beam of length 0, a beam through the camera position, a beam
    behind the back wall (past every tfar), and an upright beam beside the box where camera rays pass that miss the scene."""
    sc = orc.Scene(sd)
    cam, central = sc.camera_generate(sd.width / 2, sd.height / 2)
    cam, central = np.asarray(cam, np.float32), np.asarray(central, np.float32)
    rs = np.random.RandomState(12)
    o = rs.uniform((-0.9, 0.1, -0.9), (0.9, 1.9, 0.9), (24, 3)).astype(np.float32)
    d = rs.normal(size=(24, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    cloud = R.beam_words(o, rs.uniform(0.2, 1.2, 24).astype(np.float32), d, rs.uniform(0.5, 4.0, (24, 3)), path=np.arange(24) % 7)
    x = np.asarray([1.0, 0.0, 0.0], np.float32)
    special = np.concatenate([
        R.beam_words([(0.1, 1.0, 0.5)], 1.0, [central], [(1.0, 1.0, 1.0)]),
        R.beam_words([(0.3, 0.7, 0.2)], 0.0, [(0.0, 1.0, 0.0)], [(5.0, 5.0, 5.0)]),
        R.beam_words([cam - x * np.float32(0.5)], 1.0, [x], [(2.0, 1.0, 0.5)]),
        R.beam_words([(-0.5, 1.0, -1.5)], 1.0, [x], [(9.0, 9.0, 9.0)]),
        R.beam_words([(1.3, 0.2, 0.0)], 1.6, [(0.0, 0.6, 0.8)], [(3.0, 2.0, 1.0)]),
    ])
    return sc, np.concatenate([cloud[:12], special, cloud[12:]])


@pytest.mark.parametrize("streaming", [False, True])
def test_hand_made_beams(built, streaming):
    sd = scenes.cbox_medium(40, 24, 1.0)
    sc, words = _hand_made(sd)
    ctx = _context(sd, streaming)
    bmap = ctx.beam_map_from_words(words, 7, 0.1)
    seeds = api.IndependentSampler(8).block_seeds(sd.width, sd.height)
    img, st, detail = _render_both(sd, ctx, sc, words, 7, bmap, seeds, 3, 0.1)
    assert st["beams_accepted"] > 0 and img.any()
    miss = detail["tfar"] == R.F32_MAX
    assert miss.any() and detail["c"][miss].any()                 # rays that miss the scene, and gather on their way
    nan = words.copy()
    nan[3, 5] = np.float32("nan").view(np.uint32)
    with pytest.raises(api.RustlightError) as e:
        ctx.beam_map_from_words(nan, 7, 0.1)
    assert e.value.code == RL_ERR_INVALID_ARGUMENT
    with pytest.raises(api.RustlightError) as e:
        ctx.beam_map_from_words(words, 0, 0.1)                    # no light path to normalise by
    assert e.value.code == RL_ERR_INVALID_ARGUMENT


def test_refused_inputs(built):
    plain = _context(scenes.cbox(16, 16))                         # no medium
    words = R.beam_words([(0.0, 1.0, 0.0)], 1.0, [(1.0, 0.0, 0.0)], [(1.0, 1.0, 1.0)])
    with pytest.raises(api.RustlightError) as e:
        plain.beam_map_from_words(words, 1, 0.1)
    assert e.value.code == api.RL_ERR_UNSUPPORTED
    sd = scenes.cbox_medium(16, 16, 1.0)
    ctx, other = _context(sd), _context(sd)
    s = api.IndependentSampler(0)
    beams, _ = ctx.beam_generate(s, 16)
    for radius in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(api.RustlightError) as e:
            ctx.beam_map(beams, radius)
        assert e.value.code == RL_ERR_INVALID_ARGUMENT, radius
    with pytest.raises(api.RustlightError) as e:
        other.beam_map(beams, 0.2)                                # a set from another context
    assert e.value.code == RL_ERR_INVALID_ARGUMENT
    bmap = ctx.beam_map(beams, 0.2)
    seeds = s.block_seeds(16, 16)
    with pytest.raises(api.RustlightError) as e:
        other.render_beams(bmap, seeds)                           # a map from another context
    assert e.value.code == RL_ERR_INVALID_ARGUMENT
    for kw, code in (({"spp": (1 << 22) + 1}, api.RL_ERR_UNSUPPORTED), ({"spp": 0}, RL_ERR_INVALID_ARGUMENT),
                     ({"shard_index": 2, "shard_count": 2}, RL_ERR_INVALID_ARGUMENT)):
        with pytest.raises(api.RustlightError) as e:
            ctx.render_beams(bmap, seeds, **kw)
        assert e.value.code == code, kw


def test_integrator_compute(built):
    """IntegratorPhotonBeams::compute is the sequence of _exact: generate, map, block seeds from the sampler the generation leaves, render."""
    sd = scenes.cbox_medium(24, 16, 1.0)
    for streams in api.LIGHT_STREAMS:
        integ = api.IntegratorPhotonBeams(nb_primitive=100, radius=0.1, light_streams=streams)
        img = integ.compute(api.IndependentSampler(9), api.Scene(sd), 2)
        want, st, _ = _exact(sd, seed=9, nb=100, spp=2, radius=0.1, streams=streams)
        np.testing.assert_array_equal(img, want)
        assert integ.last_stats["beams_accepted"] == st["beams_accepted"]


def test_cli_renders_what_the_api_renders(built, tmp_path):
    """`photon-beams` goes through the C++ mirror (integrator.hpp: IntegratorPhotonBeams::compute): the same bytes as the Python mirror."""
    scn = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "cbox.pbrt")
    out = str(tmp_path / "out.pfm")
    args = [cli.EXE, scn, "-n", "2", "-r", "independent:7", "-m", "1.0", "-o", out]
    for extra, streams in (([], "reference"), (["--light-streams", "per-path"], "per_path")):
        r = subprocess.run(args + ["photon-beams", "--nb-primitive", "200", "--radius", "0.1", "-m", "6", "-r", "3"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        img = api.load_pfm(out)
        scene = api.Scene.load(scn)
        scene.set_medium((0.0,) * 3, (1.0,) * 3)
        want = api.IntegratorPhotonBeams(nb_primitive=200, max_depth=6, rr_depth=3, radius=0.1, light_streams=streams).compute(api.IndependentSampler(7), scene, 2)
        assert img.shape == want.shape and want.any()
        np.testing.assert_array_equal(img, want)
