"""The photon beams' beam pass (rl_beam_generate, rl_beam_generate_paths, kernels/beamgen.hip.h) held to the oracle's light paths, which know nothing of beams.

On a box whose BSDFs are all non-smooth, with a medium, Scene.vpl_generate(state, 1, .., VPL_ALL) shoots exactly one light path (tests/vpl_paths_restatement.py)
and stores one record per vertex: the light vertex, then the vertex every traced edge ends in.  Beam j of the path is the edge from vertex j to vertex j + 1, so
for every path, exactly: the beam count is the oracle's extension-ray count; o and radiance of beam j are record j's position and radiance; from_surface is
(record j is no volume record); for a volume successor d = -d_in of record j + 1 and o + d * length (multiply, add, in f32) is its position; for a surface
successor length is the oracle's trace distance along (o, d) and to_local(frame, -d) is the record's wi.  With a glass and a mirror mesh the smooth vertices
store no record, and the chain is held instead: beam j + 1 starts where beam j ends.  One process, no child."""
import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests.gather_exact import GEN_KEYS
from tests.scene_helpers import context as _context, glass_and_mirror

pytestmark = pytest.mark.gpu

F32 = np.float32
KIND_VOLUME = 1
SEED = 5


def _dot(a, b):
    return F32(F32(F32(a[0] * b[0]) + F32(a[1] * b[1])) + F32(a[2] * b[2]))


def _oracle_paths(sc, seed, variant, per_path, stop, max_depth=None, rr_depth=0):
    """The light paths shot until stop(paths) holds: [(records [n, 24] u32, stats)], and the main sampler's state afterwards."""
    main = orc.Rng(seed, variant)
    state = np.array(list(main.state), np.uint64)
    paths = []
    while not stop(paths):
        start = np.array(list(orc.Rng(main.next_u64(), variant).state), np.uint64) if per_path else state
        rec, n, after, st = sc.vpl_generate(start, 1, max_depth, rr_depth, orc.VPL_ALL)
        assert n == 1
        paths.append((rec.copy(), st))
        if not per_path:
            state = after
    return paths, (np.array(list(main.state), np.uint64) if per_path else state)


def _beams_stored(paths):
    return sum(st["extension_rays"] for _, st in paths)


def _check_path(sc, k, rec, st, beams):
    """Beams of path k (a structured array) against the path's vertex records."""
    assert beams.shape[0] == st["extension_rays"] == rec.shape[0] - 1, k
    f = rec.view(np.float32)
    for j, b in enumerate(beams):
        what = (k, j)
        assert int(b["path"]) == k, what
        np.testing.assert_array_equal(b["o"].view(np.uint32), rec[j, 4:7], err_msg=str(what))
        np.testing.assert_array_equal(b["radiance"].view(np.uint32), rec[j, 7:10], err_msg=str(what))
        assert int(b["flags"]) == (0 if rec[j, 0] == KIND_VOLUME else 1), what
        o, d, length = b["o"], b["d"], b["length"]
        if rec[j + 1, 0] == KIND_VOLUME:
            np.testing.assert_array_equal(d.view(np.uint32), (-f[j + 1, 10:13]).view(np.uint32), err_msg=str(what))
            np.testing.assert_array_equal((o + d * length).view(np.uint32), rec[j + 1, 4:7], err_msg=str(what))
        else:
            hit = sc.trace_full(o, d)
            assert hit is not None and F32(hit["t"]).view(np.uint32) == length.view(np.uint32), what
            x, y, z = f[j + 1, 15:18], f[j + 1, 18:21], f[j + 1, 21:24]
            wi = np.array([_dot(-d, x), _dot(-d, y), _dot(-d, z)], np.float32)          # to_local(frame, -d)
            np.testing.assert_array_equal(wi.view(np.uint32), rec[j + 1, 10:13], err_msg=str(what))


def _check_set(sc, ctx, seed, variant, nb, per_path, paths, state_after, max_depth=None, rr_depth=0):
    sampler = api.IndependentSampler(seed, variant)
    beams, gst = ctx.beam_generate(sampler, nb, max_depth, rr_depth, "per_path" if per_path else "reference")
    recs = beams.records()
    n_beams, n_paths = beams.info()
    assert n_paths == len(paths) and n_beams == recs.shape[0] == _beams_stored(paths) >= nb
    at = 0
    for k, (rec, st) in enumerate(paths):
        n = st["extension_rays"]
        _check_path(sc, k, rec, st, recs[at:at + n])
        at += n
    np.testing.assert_array_equal(np.array(list(sampler.s.s), np.uint64), state_after)
    assert gst["camera_samples"] == len(paths)
    for key in GEN_KEYS[1:]:
        assert gst[key] == sum(st[key] for _, st in paths), key
    return beams.words()


@pytest.fixture(scope="module")
def box(built):
    sd = scenes.cbox_medium(16, 16, 1.0)
    return sd, orc.Scene(sd), _context(sd)


@pytest.mark.parametrize("per_path", [False, True])
def test_beams_are_the_edges_of_the_oracles_paths(box, per_path):
    sd, sc, ctx = box
    paths, after = _oracle_paths(sc, SEED, 0, per_path, lambda p: _beams_stored(p) >= 150)
    assert len(paths) >= 10 and max(st["extension_rays"] for _, st in paths) >= 6
    kinds = np.concatenate([rec[1:, 0] for rec, _ in paths])
    assert (kinds == KIND_VOLUME).any() and (kinds != KIND_VOLUME).any()              # both successors
    _check_set(sc, ctx, SEED, 0, 150, per_path, paths, after)


@pytest.mark.parametrize("per_path", [False, True])
def test_stop_rule(box, per_path):
    """nb_primitive = 1: one path, all of its beams; then a count the fifth path exactly reaches, and that count plus one."""
    sd, sc, ctx = box
    paths, after = _oracle_paths(sc, SEED, 1, per_path, lambda p: len(p) >= 1)
    _check_set(sc, ctx, SEED, 1, 1, per_path, paths, after)
    five, after5 = _oracle_paths(sc, SEED, 1, per_path, lambda p: len(p) >= 5)
    exact = _beams_stored(five)
    assert exact > _beams_stored(five[:4])                                            # the fifth path stores a beam
    _check_set(sc, ctx, SEED, 1, exact, per_path, five, after5)
    more, after_more = _oracle_paths(sc, SEED, 1, per_path, lambda p: _beams_stored(p) >= exact + 1)
    assert len(more) > 5
    _check_set(sc, ctx, SEED, 1, exact + 1, per_path, more, after_more)


@pytest.mark.parametrize("per_path", [False, True])
def test_max_depth_2_stores_one_beam_per_path_from_the_light(box, per_path):
    sd, sc, ctx = box
    paths, after = _oracle_paths(sc, 9, 0, per_path, lambda p: _beams_stored(p) >= 40, max_depth=2)
    words = _check_set(sc, ctx, 9, 0, 40, per_path, paths, after, max_depth=2)
    assert words.shape[0] == len(paths) == 40 and (words[:, 7] == 1).all()
    np.testing.assert_array_equal(words[:, 11], np.arange(40))


def test_depth_and_rr_options(box):
    sd, sc, ctx = box
    paths, after = _oracle_paths(sc, 2, 0, False, lambda p: _beams_stored(p) >= 60, max_depth=4, rr_depth=2)
    _check_set(sc, ctx, 2, 0, 60, False, paths, after, max_depth=4, rr_depth=2)


def test_per_path_beams_do_not_depend_on_the_batch(box):
    sd, sc, ctx = box
    got = []
    for batch in (None, 1, 7, 64):
        with ctx.options(vpl_batch_paths=batch):
            s = api.IndependentSampler(SEED, 0)
            beams, _ = ctx.beam_generate(s, 150, streams="per_path")
            got.append((beams.words(), beams.info(), list(s.s.s)))
    for words, info, state in got[1:]:
        np.testing.assert_array_equal(words, got[0][0])
        assert info == got[0][1] and state == got[0][2]


@pytest.mark.parametrize("per_path", [False, True])
@pytest.mark.parametrize("streaming", [False, True])
def test_chain_through_glass_and_mirror(built, per_path, streaming):
    """Smooth vertices store no record; the beams still chain: beam j + 1 starts at the oracle's hit point of beam j, or where beam j ends in the medium."""
    sd = glass_and_mirror(16, 16)
    sd.medium = scenes.Medium((0.0,) * 3, (0.3,) * 3)
    sc, ctx = orc.Scene(sd), _context(sd, streaming)
    paths, after = _oracle_paths(sc, 4, 0, per_path, lambda p: _beams_stored(p) >= 400)
    sampler = api.IndependentSampler(4, 0)
    beams, gst = ctx.beam_generate(sampler, 400, streams="per_path" if per_path else "reference")
    recs = beams.records()
    assert beams.info() == (_beams_stored(paths), len(paths))
    np.testing.assert_array_equal(np.array(list(sampler.s.s), np.uint64), after)
    for key in GEN_KEYS[1:]:
        assert gst[key] == sum(st[key] for _, st in paths), key
    at, surface_links, smooth_links = 0, 0, 0
    for k, (rec, st) in enumerate(paths):
        n = st["extension_rays"]
        mine = recs[at:at + n]
        at += n
        assert (mine["path"] == k).all() and (n == 0 or mine[0]["flags"] == 1)
        smooth_links += n - (rec.shape[0] - 1)                                          # vertices that stored no record
        for j in range(n - 1):
            a, b = mine[j], mine[j + 1]
            if b["flags"] & 1:
                hit = sc.trace_full(a["o"], a["d"])
                assert hit is not None and F32(hit["t"]).view(np.uint32) == a["length"].view(np.uint32), (k, j)
                np.testing.assert_array_equal(b["o"].view(np.uint32), np.asarray(hit["p"], np.float32).view(np.uint32), err_msg=str((k, j)))
                surface_links += 1
            else:
                np.testing.assert_array_equal(b["o"].view(np.uint32), (a["o"] + a["d"] * a["length"]).view(np.uint32), err_msg=str((k, j)))
    assert surface_links > 0 and smooth_links > 0


def test_refused_inputs(built):
    plain = _context(scenes.cbox(16, 16))                       # no medium
    with pytest.raises(api.RustlightError) as e:
        plain.beam_generate(api.IndependentSampler(0), 8)
    assert e.value.code == api.RL_ERR_UNSUPPORTED
    ctx = _context(scenes.cbox_medium(16, 16, 1.0))
    for streams in api.LIGHT_STREAMS:
        for nb in (0, api.BEAM_MAX + 1):
            with pytest.raises(api.RustlightError) as e:
                ctx.beam_generate(api.IndependentSampler(0), nb, streams=streams)
            assert e.value.code == -1, (streams, nb)
        with pytest.raises(api.RustlightError) as e:
            ctx.beam_generate(api.IndependentSampler(0), 8, max_depth=1, streams=streams)
        assert e.value.code == -1, streams
