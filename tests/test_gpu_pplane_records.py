"""The photon planes' plane pass (rl_pplane_generate, rl_pplane_generate_paths, kernels/pplanegen.hip.h) held to the beam pass and to the oracle's sampler.

The light paths are those of rl_beam_generate / rl_beam_generate_paths from the same sampler state, which tests/test_gpu_beam_records.py holds to the oracle's
light paths: one beam per traced edge.  For every path, the plane pass's surface beams and planes must be exactly pplane_restatement.convert of that path's
edges: which edges stay beams, which pairs become planes, every field bit for bit, in edge order.  length1 of a plane whose second edge scattered is that
beam's length; where the second edge hit a surface it is -ln(1 - u') / sigma_t[c] of that edge's own medium draw, which no beam record holds (nor does one say where a path's last edge ended): continued_t of every edge is taken from
orc.Rng at the draw's index in the path's stream (4 + 2 + 1 draws up to the first edge, then 2 + [1 under Russian roulette] + 1 per expansion).  The index is
confirmed twice: the same formula gives every scattered edge's length, bit for bit, and the path's draw count (the oracle's) leaves 0, 2 or 3 draws behind the
last edge's.  One process, no child."""
import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import plane_single_restatement as P
from tests import pplane_restatement as Q
from tests.gather_exact import GEN_KEYS
from tests.scene_helpers import context as _context

pytestmark = pytest.mark.gpu

SEED = 5


def _oracle_paths(sc, seed, variant, per_path, n_paths, max_depth=None, rr_depth=0):
    """The first n_paths light paths: [(start state, counters)], and the main sampler's state after them."""
    main = orc.Rng(seed, variant)
    state = np.array(list(main.state), np.uint64)
    paths = []
    for _ in range(n_paths):
        start = np.array(list(orc.Rng(main.next_u64(), variant).state), np.uint64) if per_path else state
        _, n, after, st = sc.vpl_generate(start, 1, max_depth, rr_depth, orc.VPL_ALL)
        assert n == 1
        paths.append((start, st))
        if not per_path:
            state = after
    return paths, (np.array(list(main.state), np.uint64) if per_path else state)


def _check_set(box, seed, variant, nb, per_path, max_depth=None, rr_depth=0):
    """One plane pass against the beam pass of the same sampler state.  Returns (plane records, beam records, paths shot)."""
    sd, sc, ctx = box
    streams = "per_path" if per_path else "reference"
    sigma_t = P.sigma_t_of(sd.medium)
    sampler = api.IndependentSampler(seed, variant)
    records, gst = ctx.pplane_generate(sampler, nb, max_depth, rr_depth, streams)
    planes, beams = records.records()
    n_planes, n_beams, K = records.info()
    assert planes.shape[0] == n_planes >= nb and beams.shape[0] == n_beams
    # the beam pass over at least the same paths
    edges_all, _ = ctx.beam_generate(api.IndependentSampler(seed, variant), 40 * K + 64, max_depth, rr_depth, streams)
    edge_recs = edges_all.records()
    assert edges_all.info()[1] >= K
    paths, state_after = _oracle_paths(sc, seed, variant, per_path, K, max_depth, rr_depth)
    pw, bw = records.words()
    at_p = at_b = 0
    surface_end_planes = scattered_planes = 0
    for k, (start, st) in enumerate(paths):
        mine = edge_recs[edge_recs["path"] == k]
        n = mine.shape[0]
        assert n == st["extension_rays"], k
        idx = Q.medium_draw_indices(n, rr_depth)
        assert n == 0 or st["rng_draws"] - (idx[-1] + 1) in (0, 2, 3), (k, st["rng_draws"], idx)
        rng = orc.Rng.from_state([int(v) for v in start])
        draws = [rng.next_f32() for _ in range(idx[-1] + 1 if n else 0)]
        ct = [Q.continued_t(draws[i], sigma_t) for i in idx]
        for j in range(n):                                        # an edge that scattered: its length is its own draw's distance
            if j + 1 < n and not (mine[j + 1]["flags"] & 1):
                assert ct[j].view(np.uint32) == mine[j]["length"].view(np.uint32), (k, j)
            else:                                                 # it hit a surface, or is the path's last: the draw reached at least as far
                assert ct[j] >= mine[j]["length"], (k, j)
        edges = Q.edges_of_beams(mine, lambda j: ct[j])
        want_b, want_p = Q.convert(edges, k)
        np.testing.assert_array_equal(bw[at_b:at_b + want_b.shape[0]], want_b, err_msg=f"beams of path {k}")
        np.testing.assert_array_equal(pw[at_p:at_p + want_p.shape[0]], want_p, err_msg=f"planes of path {k}")
        for w in want_p:
            e2 = edges[int(w[15]) + 1]
            if e2["ct"] > e2["length"]:
                surface_end_planes += 1
            else:
                scattered_planes += 1
        at_b += want_b.shape[0]
        at_p += want_p.shape[0]
        if k < K - 1:
            assert at_p < nb, k                                   # `while planes.len() < nb_primitive`: no path is shot past the count
    assert (at_p, at_b) == (n_planes, n_beams)
    np.testing.assert_array_equal(np.array(list(sampler.s.s), np.uint64), state_after)
    assert gst["camera_samples"] == K
    for key in GEN_KEYS[1:]:
        assert gst[key] == sum(st[key] for _, st in paths), key
    return planes, beams, K, (surface_end_planes, scattered_planes)


@pytest.fixture(scope="module")
def box(built):
    sd = scenes.cbox_medium(16, 16, 1.0)
    return sd, orc.Scene(sd), _context(sd)


@pytest.mark.parametrize("per_path", [False, True])
def test_records_are_the_conversion_of_the_beam_passes_edges(box, per_path):
    planes, beams, K, (surface_end, scattered) = _check_set(box, SEED, 0, 150, per_path)
    assert K >= 10 and surface_end > 0 and scattered > 0          # both kinds of length1
    surf = (beams["flags"] & 1) == 1
    assert surf.any() and (~surf).any()                           # beams from surfaces and the light, and beams from the medium
    assert (planes["zero"] == 0).all() and (planes["length1"] > 0).all()


@pytest.mark.parametrize("per_path", [False, True])
def test_stop_rule(box, per_path):
    """nb_primitive = 1: the paths up to the first that holds a plane, all of its records; then a count a path exactly reaches, and that count plus one."""
    planes, _, K, _ = _check_set(box, SEED, 1, 1, per_path)
    assert (planes["path"] == K - 1).all()
    many, _, K5, _ = _check_set(box, SEED, 1, 30, per_path)
    ends = np.cumsum(np.bincount(many["path"], minlength=K5))    # planes stored once each path is done
    exact = int(ends[np.nonzero(np.diff(ends, prepend=0))[0][2]])      # the count the third plane-storing path reaches
    got, _, K_exact, _ = _check_set(box, SEED, 1, exact, per_path)
    assert got.shape[0] == exact
    more, _, K_more, _ = _check_set(box, SEED, 1, exact + 1, per_path)
    assert K_more > K_exact and more.shape[0] > exact


@pytest.mark.parametrize("per_path", [False, True])
def test_max_depth_4_gives_planes_from_the_first_volume_vertex_only(box, per_path):
    planes, _, _, _ = _check_set(box, 9, 0, 40, per_path, max_depth=4)
    assert (planes["edge"] == 1).all()


def test_depth_and_rr_options(box):
    _check_set(box, 2, 0, 60, False, max_depth=6, rr_depth=3)
    _check_set(box, 2, 0, 60, True, max_depth=None, rr_depth=None)


def test_per_path_records_do_not_depend_on_the_batch(box):
    sd, sc, ctx = box
    got = []
    for batch in (None, 1, 7, 64):
        with ctx.options(vpl_batch_paths=batch):
            s = api.IndependentSampler(SEED, 0)
            records, _ = ctx.pplane_generate(s, 150, streams="per_path")
            got.append((records.words(), records.info(), list(s.s.s)))
    for words, info, state in got[1:]:
        np.testing.assert_array_equal(words[0], got[0][0][0])
        np.testing.assert_array_equal(words[1], got[0][0][1])
        assert info == got[0][1] and state == got[0][2]


def test_streamed_scene_gives_the_same_records(box):
    sd, sc, ctx = box
    streamed = _context(sd, True)
    for streams in api.LIGHT_STREAMS:
        a, _ = ctx.pplane_generate(api.IndependentSampler(SEED), 100, streams=streams)
        b, _ = streamed.pplane_generate(api.IndependentSampler(SEED), 100, streams=streams)
        for x, y in zip(a.words(), b.words()):
            np.testing.assert_array_equal(x, y)
        assert a.info() == b.info()


def test_refused_inputs(built):
    plain = _context(scenes.cbox(16, 16))                       # no medium
    with pytest.raises(api.RustlightError) as e:
        plain.pplane_generate(api.IndependentSampler(0), 8)
    assert e.value.code == api.RL_ERR_UNSUPPORTED
    ctx = _context(scenes.cbox_medium(16, 16, 1.0))
    for streams in api.LIGHT_STREAMS:
        for nb in (0, api.BEAM_MAX + 1):
            with pytest.raises(api.RustlightError) as e:
                ctx.pplane_generate(api.IndependentSampler(0), nb, streams=streams)
            assert e.value.code == -1, (streams, nb)
        for max_depth in (1, 2, 3):                             # no light path holds a plane: the reference never stops shooting
            s = api.IndependentSampler(0)
            before = list(s.s.s)
            with pytest.raises(api.RustlightError) as e:
                ctx.pplane_generate(s, 8, max_depth=max_depth, streams=streams)
            assert e.value.code == -1 and list(s.s.s) == before, (streams, max_depth)
    # a closed scene (the open box lets light paths out into the endless medium, where every edge scatters) with a medium so thin that the surface beams
    # pass RL_BEAM_MAX + 2048 before 64 planes exist: refused, with the medium named
    thin = _context(_closed_box(1e-4))
    for streams in api.LIGHT_STREAMS:
        s = api.IndependentSampler(0)
        before = list(s.s.s)
        with pytest.raises(api.RustlightError) as e:
            thin.pplane_generate(s, 64, streams=streams)
        assert e.value.code == api.RL_ERR_UNSUPPORTED and "medium" in str(e.value) and list(s.s.s) == before, streams


def _closed_box(sigma_s):
    """The box inside a black cube of side 40: no light path leaves the scene."""
    sd = scenes.cbox_medium(16, 16, sigma_s)
    c, h = np.asarray([0.0, 1.0, 0.0], np.float32), np.float32(20.0)
    v = np.asarray([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32) * h + c
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    idx = np.asarray([t for a, b, cc, d in quads for t in ((a, b, cc), (a, cc, d))], np.uint32)
    sd.meshes.append(scenes.MeshData("Shell", v, idx, None, None, scenes.matte((0.0, 0.0, 0.0))))
    return sd
