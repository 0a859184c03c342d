"""The photon planes' gather (rl_pplane_map_build / rl_render_photon_planes, kernels/pplane.hip.h) held bit for bit to the numpy restatement of the reference's
text (tests/pplane_restatement.py): the image (assert_array_equal) and every counter, over LDS-staged and streamed BVHs, grey, coloured and Henyey-Greenstein
media, ragged and one-pixel-wide frames, spp 1 and 3 (at spp 3 the image depends on beams and planes being added per sample, not per tree), shards of 2 and 3,
both stream modes of the plane pass, a plane set whose tree root is a leaf, the plane tree from the host and from the device kernels, and hand-made records.
The records come from the device's own plane pass, which tests/test_gpu_pplane_records.py holds to the beam pass and the oracle's sampler.  The refused inputs
return their codes; the CLI writes the bytes the API renders.  One process; only the CLI test starts a child."""
import os
import subprocess

import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import cli
from tests import beam_restatement as R
from tests import pplane_restatement as Q
from tests.beam_half_cases import assert_beam_half
from tests.photon_tree_cases import assert_trees_equal
from tests.scene_helpers import context as _context
from tests.test_gpu_gather_edges import coloured

pytestmark = pytest.mark.gpu

RL_ERR_INVALID_ARGUMENT = -1


def _render_both(sd, ctx, sc, beams, planes, n_paths, pmap, seeds, spp, radius, variant=0, shard=(0, 1)):
    img, st = ctx.render_photon_planes(pmap, seeds, spp, variant, *shard)
    ref_img, ref_st, detail = Q.render(sc, sd, beams, planes, n_paths, seeds, spp, radius, variant, *shard)
    np.testing.assert_array_equal(img, ref_img)
    for k in Q.KEYS:
        assert st[k] == ref_st[k], k
    return img, st, detail


def _packed_planes(planes, order):
    f = planes[order].view(np.float32)
    want = np.zeros((planes.shape[0], 16), np.float32)
    want[:, 0:3], want[:, 3] = f[:, 0:3], f[:, 9]
    want[:, 4:7], want[:, 7] = f[:, 3:6], f[:, 10]
    want[:, 8:11] = f[:, 6:9]
    want[:, 12:15] = f[:, 11:14]
    return want


def _check_map(pmap, beams, planes, n_paths, radius):
    """Both trees and both element arrays of a map against the host-only builds."""
    n_sub, n_beam_nodes = assert_beam_half(pmap.read("beams"), beams, radius, "beam tree")
    pboxes, plinks, porder = api.plane_tree_build(planes)
    got = pmap.read("planes")
    assert_trees_equal(got[:2], (pboxes, plinks), "plane tree")
    np.testing.assert_array_equal(got[2].view(np.uint32), _packed_planes(planes, porder).view(np.uint32))
    assert pmap.info() == (beams.shape[0], n_sub, n_beam_nodes, planes.shape[0], pboxes.shape[0], n_paths, pytest.approx(radius))


def _exact(sd, seed=3, nb=60, spp=3, radius=0.1, max_depth=None, rr_depth=0, variant=0, streaming=False, streams="reference", options=None):
    """Plane pass, map and gather of one scene: the map against the host-only builds, image and counters against the restatement."""
    ctx, sc = _context(sd, streaming), orc.Scene(sd)
    for k, v in (options or {}).items():
        ctx.set_option(k, v)
    sampler = api.IndependentSampler(seed, variant)
    records, _ = ctx.pplane_generate(sampler, nb, max_depth, rr_depth, streams)
    (planes, beams), (n_planes, n_beams, n_paths) = records.words(), records.info()
    assert planes.shape[0] == n_planes >= nb and beams.shape[0] == n_beams
    pmap = ctx.pplane_map(records, radius)
    _check_map(pmap, beams, planes, n_paths, radius)
    seeds = sampler.block_seeds(sd.width, sd.height)
    img, st, detail = _render_both(sd, ctx, sc, beams, planes, n_paths, pmap, seeds, spp, radius, variant)
    assert st["beams_accepted"] > 0 and st["planes_visible"] > 0 and img.any()          # no case passes empty
    return img, st, detail


@pytest.mark.parametrize("streaming", [False, True])
@pytest.mark.parametrize("streams", ["reference", "per_path"])
def test_grey_medium(built, streaming, streams):
    _, st, detail = _exact(scenes.cbox_medium(40, 24, 1.0), streaming=streaming, streams=streams)
    assert (detail["tfar"] == R.F32_MAX).any()                    # camera rays that miss the scene still gather
    assert st["planes_visible"] < st["planes_intersected"]        # and some planes are hidden from their ray


def test_beams_and_planes_are_added_per_sample(built):
    """At spp 3 the reference's sum over samples of (beams + planes) differs in f32 from the sum of two images: the case that needs one kernel."""
    _, _, detail = _exact(scenes.cbox_medium(40, 24, 1.0))
    c, cb = detail["c"], detail["c_beams"]
    cp = np.zeros_like(c)
    Q.gather_planes(detail["plane_tree"], detail["planes"], detail["o"], detail["d"], detail["tfar"], cp)       # the planes alone, from black
    two = sum(cb[s::3] for s in range(3)) + sum(cp[s::3] for s in range(3))
    one = sum(c[s::3] for s in range(3))
    assert (two.view(np.uint32) != one.view(np.uint32)).any()


@pytest.mark.parametrize("streaming", [False, True])
def test_coloured_medium(built, streaming):
    img, _, _ = _exact(coloured(40, 24), streaming=streaming)
    m = [float(np.mean(img[..., k], dtype=np.float64)) for k in range(3)]
    assert m[0] != m[1] and m[1] != m[2] and m[0] != m[2] and min(m) > 0.0, m


def test_henyey_greenstein_medium_gathers_isotropically(built):
    """A plane's phase function is Isotropic whatever the medium's is (vol_primitives.rs:410): the restatement has no other."""
    _exact(scenes.cbox_medium(40, 24, 1.0, g=0.6), streaming=False)
    _exact(coloured(24, 16, g=-0.4), nb=40, spp=1, streaming=True)


@pytest.mark.parametrize("w,h,spp", [(40, 24, 1), (1, 33, 3), (33, 1, 3), (33, 20, 1)])
def test_frames_and_spp(built, w, h, spp):
    _exact(scenes.cbox_medium(w, h, 1.0), nb=40, spp=spp, radius=0.3, variant=1 if w == 1 else 0)


def test_depth_options_and_a_root_that_is_a_leaf(built):
    _exact(scenes.cbox_medium(24, 16, 1.0), seed=2, nb=50, spp=2, max_depth=5, rr_depth=2, radius=0.2)
    # nb_primitive = 1 under max_depth = 4: the first path with a plane stores one or two, so the plane tree is one leaf
    _, _, detail = _exact(scenes.cbox_medium(24, 16, 1.0), seed=6, nb=1, spp=2, radius=0.5, max_depth=4)
    nodes = detail["plane_tree"]["nodes"]
    assert len(nodes) == 1 and nodes[0]["left"] is None and 1 <= nodes[0]["count"] <= 4


@pytest.mark.parametrize("shards", [2, 3])
def test_shards_sum_to_the_frame(built, shards):
    sd = scenes.cbox_medium(40, 40, 1.0)
    ctx, sc = _context(sd), orc.Scene(sd)
    sampler = api.IndependentSampler(4)
    records, _ = ctx.pplane_generate(sampler, 50)
    pmap = ctx.pplane_map(records, 0.1)
    seeds = sampler.block_seeds(sd.width, sd.height)
    whole, st = ctx.render_photon_planes(pmap, seeds, 2)
    (planes, beams), n_paths = records.words(), records.info()[2]
    parts = [_render_both(sd, ctx, sc, beams, planes, n_paths, pmap, seeds, 2, 0.1, 0, (k, shards)) for k in range(shards)]
    assert whole.any()
    np.testing.assert_array_equal(sum(p[0] for p in parts), whole)
    for k in Q.KEYS:
        assert sum(p[1][k] for p in parts) == st[k], k


def test_host_and_device_plane_tree_give_the_same_map(built):
    """Option pplane_tree_device: the plane tree from the kernels of rl_plane_map_build_device, byte for byte the host's (_check_map reads both)."""
    sd = scenes.cbox_medium(24, 16, 1.0)
    host = _exact(sd, seed=5, nb=300, spp=1)
    dev = _exact(sd, seed=5, nb=300, spp=1, options={"pplane_tree_device": 1})
    np.testing.assert_array_equal(host[0], dev[0])
    assert host[1]["nodes_entered"] == dev[1]["nodes_entered"]
    # ... and over several workgroups' worth of global levels
    _exact(sd, seed=5, nb=300, spp=1, options={"pplane_tree_device": 1, "plane_tree_group_planes": 16})


# ---- hand-made records through rl_pplane_map_build_words
def _hand_made(sd):
    """A cloud of planes and beams in and beside the box, then: a degenerate plane (d0 = d1: |det| < 1e-5 for every ray), a plane of length0 = 0, a plane the
    central camera ray lies in, a plane behind the back wall (past every tfar) and a plane beside the box where camera rays pass that miss the scene."""
    sc = orc.Scene(sd)
    cam, central = sc.camera_generate(sd.width / 2, sd.height / 2)
    central = np.asarray(central, np.float32)
    rs = np.random.RandomState(12)

    def dirs(n):
        d = rs.normal(size=(n, 3))
        return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)

    o = rs.uniform((-0.9, 0.1, -0.9), (0.9, 1.9, 0.9), (20, 3)).astype(np.float32)
    cloud = Q.plane_words(o, dirs(20), dirs(20), rs.uniform(0.2, 1.2, 20), rs.uniform(0.2, 1.2, 20), rs.uniform(0.5, 4.0, (20, 3)), np.arange(20) % 7, 1)
    x, y = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    special = np.concatenate([
        Q.plane_words([(0.1, 1.0, 0.5)], [x], [x], 1.0, 1.0, [(1.0, 1.0, 1.0)]),
        Q.plane_words([(0.3, 0.7, 0.2)], [x], [y], 0.0, 1.0, [(5.0, 5.0, 5.0)]),
        Q.plane_words([(0.0, 1.0, 0.5)], [central], [y], 1.0, 1.0, [(2.0, 1.0, 0.5)]),
        Q.plane_words([(-0.5, 0.5, -1.5)], [x], [y], 1.0, 1.0, [(9.0, 9.0, 9.0)]),
        Q.plane_words([(1.3, 0.2, 0.0)], [y], [(0.0, 0.6, 0.8)], 1.6, 1.0, [(3.0, 2.0, 1.0)]),
    ])
    ob = rs.uniform((-0.9, 0.1, -0.9), (0.9, 1.9, 0.9), (12, 3)).astype(np.float32)
    beams = R.beam_words(ob, rs.uniform(0.2, 1.2, 12).astype(np.float32), dirs(12), rs.uniform(0.5, 4.0, (12, 3)), path=np.arange(12) % 7)
    return sc, beams, np.concatenate([cloud[:10], special, cloud[10:]])


@pytest.mark.parametrize("streaming", [False, True])
def test_hand_made_records(built, streaming):
    sd = scenes.cbox_medium(40, 24, 1.0)
    sc, beams, planes = _hand_made(sd)
    ctx = _context(sd, streaming)
    pmap = ctx.pplane_map_from_words(beams, planes, 7, 0.1)
    _check_map(pmap, beams, planes, 7, 0.1)
    seeds = api.IndependentSampler(8).block_seeds(sd.width, sd.height)
    img, st, detail = _render_both(sd, ctx, sc, beams, planes, 7, pmap, seeds, 3, 0.1)
    assert st["beams_accepted"] > 0 and st["planes_visible"] > 0 and img.any()
    miss = detail["tfar"] == R.F32_MAX
    assert miss.any() and detail["c"][miss].any()                 # rays that miss the scene, and gather on their way
    for bad_b, bad_p in ((3, None), (None, 4)):
        b, p = beams.copy(), planes.copy()
        if bad_b is not None:
            b[bad_b, 5] = np.float32("nan").view(np.uint32)
        else:
            p[bad_p, 1] = np.float32("inf").view(np.uint32)
        with pytest.raises(api.RustlightError) as e:
            ctx.pplane_map_from_words(b, p, 7, 0.1)
        assert e.value.code == RL_ERR_INVALID_ARGUMENT
    with pytest.raises(api.RustlightError) as e:
        ctx.pplane_map_from_words(beams, planes, 0, 0.1)          # no light path to normalise by
    assert e.value.code == RL_ERR_INVALID_ARGUMENT
    for word in (16, 17):                                         # the words both tree builds take for 0
        p = planes.copy()
        p[2, word] = 1
        with pytest.raises(api.RustlightError) as e:
            ctx.pplane_map_from_words(beams, p, 7, 0.1)
        assert e.value.code == RL_ERR_INVALID_ARGUMENT, word
    with ctx.options(pplane_tree_device=1):                       # and the device build of the same records: the same bytes
        _check_map(ctx.pplane_map_from_words(beams, planes, 7, 0.1), beams, planes, 7, 0.1)


def test_refused_inputs(built):
    plain = _context(scenes.cbox(16, 16))                         # no medium
    sd = scenes.cbox_medium(16, 16, 1.0)
    _, beams, planes = _hand_made(sd)
    with pytest.raises(api.RustlightError) as e:
        plain.pplane_map_from_words(beams, planes, 1, 0.1)
    assert e.value.code == api.RL_ERR_UNSUPPORTED
    ctx, other = _context(sd), _context(sd)
    s = api.IndependentSampler(0)
    records, _ = ctx.pplane_generate(s, 16)
    for radius in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(api.RustlightError) as e:
            ctx.pplane_map(records, radius)
        assert e.value.code == RL_ERR_INVALID_ARGUMENT, radius
    with pytest.raises(api.RustlightError) as e:
        other.pplane_map(records, 0.2)                            # a set from another context
    assert e.value.code == RL_ERR_INVALID_ARGUMENT
    pmap = ctx.pplane_map(records, 0.2)
    seeds = s.block_seeds(16, 16)
    with pytest.raises(api.RustlightError) as e:
        other.render_photon_planes(pmap, seeds)                   # a map from another context
    assert e.value.code == RL_ERR_INVALID_ARGUMENT
    for kw, code in (({"spp": (1 << 22) + 1}, api.RL_ERR_UNSUPPORTED), ({"spp": 0}, RL_ERR_INVALID_ARGUMENT),
                     ({"shard_index": 2, "shard_count": 2}, RL_ERR_INVALID_ARGUMENT)):
        with pytest.raises(api.RustlightError) as e:
            ctx.render_photon_planes(pmap, seeds, **kw)
        assert e.value.code == code, kw


def test_integrator_compute(built):
    """IntegratorPhotonPlanes::compute is the sequence of _exact: generate, map, block seeds from the sampler the generation leaves, render."""
    sd = scenes.cbox_medium(24, 16, 1.0)
    for streams in api.LIGHT_STREAMS:
        integ = api.IntegratorPhotonPlanes(nb_primitive=50, radius=0.1, light_streams=streams)
        img = integ.compute(api.IndependentSampler(9), api.Scene(sd), 2)
        want, st, _ = _exact(sd, seed=9, nb=50, spp=2, radius=0.1, streams=streams)
        np.testing.assert_array_equal(img, want)
        assert integ.last_stats["planes_visible"] == st["planes_visible"]


def test_cli_renders_what_the_api_renders(built, tmp_path):
    """`photon-planes` goes through the C++ mirror (integrator.hpp: IntegratorPhotonPlanes::compute): the same bytes as the Python mirror."""
    scn = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "cbox.pbrt")
    out = str(tmp_path / "out.pfm")
    args = [cli.EXE, scn, "-n", "2", "-r", "independent:7", "-m", "1.0", "-o", out]
    for extra, streams in (([], "reference"), (["--light-streams", "per-path"], "per_path")):
        r = subprocess.run(args + ["photon-planes", "--nb-primitive", "100", "--radius", "0.1", "-m", "6", "-r", "3"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        img = api.load_pfm(out)
        scene = api.Scene.load(scn)
        scene.set_medium((0.0,) * 3, (1.0,) * 3)
        want = api.IntegratorPhotonPlanes(nb_primitive=100, max_depth=6, rr_depth=3, radius=0.1, light_streams=streams).compute(api.IndependentSampler(7), scene, 2)
        assert img.shape == want.shape and want.any()
        np.testing.assert_array_equal(img, want)
