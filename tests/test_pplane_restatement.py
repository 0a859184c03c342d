"""The photon planes without a GPU: the numpy restatement (tests/pplane_restatement.py) against a literal recursive transcription of convert_beams(true, ..) /
convert_planes over explicit vertex and edge lists, against a scalar walk of the two-tree gather, and against one closed form; then the host's plane tree over
the new records against the restatement's, the depth limit below which no plane exists, and what the fixtures hold."""
import math
import types

import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import beam_restatement as R
from tests import bre_restatement as B
from tests import plane_single_restatement as P
from tests import pplane_restatement as Q
from tests.photon_tree_cases import assert_trees_equal
from tests.test_beam_restatement import _color_times, _cross, _dot, _medium, _random_beams, _random_rays, _scalar_gather

F32 = np.float32


# ---- convert_beams(true, ..) / convert_planes (vol_primitives.rs:376-523), transcribed over a Path of explicit vertices and edges
def _path_of(kinds, rs):
    """A chain path: kinds[i] in "LSV" is vertex i (light, surface, volume); vertex i < len - 1 was expanded with edge i.  Random geometry and weights."""
    vertices, edges = [], []
    for i, k in enumerate(kinds):
        vertices.append({"kind": k, "pos": rs.uniform(-1, 1, 3).astype(np.float32), "edge_out": [i] if i + 1 < len(kinds) else []})
    for i in range(len(kinds) - 1):
        d = rs.normal(size=3)
        dist = F32(rs.uniform(0.1, 2.0))
        on_surface = kinds[i + 1] == "S"
        edges.append({"d": (d / np.linalg.norm(d)).astype(np.float32), "dist": dist, "continued_t": F32(dist * F32(rs.uniform(1.1, 3.0))) if on_surface else dist,
                      "vertices": (i, i + 1), "weight": rs.uniform(0.2, 1.5, 3).astype(np.float32), "rr_weight": F32(rs.uniform(1.0, 2.0))})
    return {"vertices": vertices, "edges": edges}


def _next_vertices(path, vid):
    return [(e, path["edges"][e]["vertices"][1]) for e in path["vertices"][vid]["edge_out"]]


def _convert_beams(path, vid, beams, flux):
    v = path["vertices"][vid]
    if v["kind"] in "SL":                                         # Vertex::Surface / Vertex::Light: always push
        for e in v["edge_out"]:
            edge = path["edges"][e]
            beams.append({"o": v["pos"], "d": edge["d"], "length": edge["dist"], "radiance": flux, "from_surface": True})
    elif v["kind"] == "V":
        for e in v["edge_out"]:
            edge = path["edges"][e]
            nxt = edge["vertices"][1]
            if path["vertices"][nxt]["kind"] == "S" or not path["vertices"][nxt]["edge_out"]:      # on_surface() || !have_next_vertices()
                beams.append({"o": v["pos"], "d": edge["d"], "length": edge["dist"], "radiance": flux, "from_surface": False})
    for e, nxt in _next_vertices(path, vid):
        edge = path["edges"][e]
        _convert_beams(path, nxt, beams, _color_times((flux * edge["weight"]).astype(np.float32), edge["rr_weight"]))


def _convert_planes(path, vid, planes, flux):
    v = path["vertices"][vid]
    if v["kind"] == "V":
        for e in v["edge_out"]:
            edge = path["edges"][e]
            nxt = edge["vertices"][1]
            if path["vertices"][nxt]["kind"] != "S" and path["vertices"][nxt]["edge_out"]:
                assert len(_next_vertices(path, nxt)) == 1
                next_edge = path["edges"][_next_vertices(path, nxt)[0][0]]
                planes.append({"o": v["pos"], "d0": edge["d"], "d1": next_edge["d"], "length0": edge["continued_t"], "length1": next_edge["continued_t"],
                               "radiance": flux, "edge": e})
    for e, nxt in _next_vertices(path, vid):
        edge = path["edges"][e]
        _convert_planes(path, nxt, planes, _color_times((flux * edge["weight"]).astype(np.float32), edge["rr_weight"]))


def _chain_edges(path, root_flux):
    """The path as the device's walk sees it: one record per edge with the flux that reached its first vertex."""
    out, flux = [], root_flux
    for i, e in enumerate(path["edges"]):
        out.append({"o": path["vertices"][i]["pos"], "d": e["d"], "length": e["dist"], "from_surface": path["vertices"][i]["kind"] != "V", "radiance": flux,
                    "ct": e["continued_t"]})
        flux = _color_times((flux * e["weight"]).astype(np.float32), e["rr_weight"])
    return out


KINDS = ["L", "LS", "LV", "LVV", "LVS", "LSV", "LVVV", "LVVS", "LVSV", "LSVV", "LVVVV", "LVVSVV", "LSVVSVVV", "LVSVSVS", "LVVVVVVS", "LSSSV", "LVVVSVVVV"]


@pytest.mark.parametrize("kinds", KINDS)
def test_conversion_equals_the_recursive_transcription(kinds):
    rs = np.random.RandomState(len(kinds) * 31 + sum(map(ord, kinds)))
    path = _path_of(kinds, rs)
    root_flux = rs.uniform(1.0, 5.0, 3).astype(np.float32)
    beams, planes = [], []
    _convert_beams(path, 0, beams, root_flux)
    _convert_planes(path, 0, planes, root_flux)
    got_b, got_p = Q.convert(_chain_edges(path, root_flux), 7)
    assert got_b.shape[0] == len(beams) and got_p.shape[0] == len(planes)
    assert len(beams) + len(planes) == len(kinds) - 1            # every edge is exactly one of the two
    if beams:
        want = np.concatenate([R.beam_words([b["o"]], b["length"], [b["d"]], [b["radiance"]], b["from_surface"], 7) for b in beams])
        np.testing.assert_array_equal(got_b, want)
    if planes:
        want = np.concatenate([Q.plane_words([p["o"]], [p["d0"]], [p["d1"]], p["length0"], p["length1"], [p["radiance"]], 7, p["edge"]) for p in planes])
        np.testing.assert_array_equal(got_p, want)
    if "S" in kinds[2:] and planes:                               # a second edge that ends on a surface keeps its sampled distance
        f = got_p.view(np.float32)
        for w in got_p:
            e2 = path["edges"][int(w[15]) + 1]
            assert w.view(np.float32)[10] == e2["continued_t"]
        assert f.shape[1] == api.PLANE_WORDS


def test_no_plane_exists_within_three_vertices_beyond_the_light():
    """V2 is expanded only when 3 < max_depth: with max_depth <= 3 a path has at most the edges L -> V1 -> V2, and V2 has no edge out."""
    rs = np.random.RandomState(0)
    for kinds in ("L", "LV", "LS", "LVV", "LVS", "LSV", "LSS"):
        assert Q.convert(_chain_edges(_path_of(kinds, rs), np.ones(3, np.float32)), 0)[1].shape[0] == 0
    sd = scenes.cbox_medium(16, 16, 1.0)
    sc = orc.Scene(sd)
    state = np.array(list(orc.Rng(1).state), np.uint64)
    for _ in range(40):                                           # and the oracle's walk under max_depth = 3 never takes a third edge
        rec, n, state, st = sc.vpl_generate(state, 1, 3, 0, orc.VPL_ALL)
        assert st["extension_rays"] <= 2
    with pytest.raises(AssertionError):
        Q.generate(sd, sc, 0, 0, 4, max_depth=3)


# ---- PhotonPlane::intersection / contribute (vol_primitives.rs:295-373), one scalar float32 operation at a time
def _plane_its(pl, ro, rd, tfar):
    with np.errstate(all="ignore"):
        e0 = (pl.d0 * pl.l0).astype(np.float32)
        e1 = (pl.d1 * pl.l1).astype(np.float32)
        p = _cross(rd, e1)
        det = _dot(e0, p)
        if abs(det) < F32(1e-5):
            return None
        inv_det = F32(F32(1.0) / det)
        t = (ro - pl.o).astype(np.float32)
        t0 = F32(_dot(t, p) * inv_det)
        if t0 < 0 or t0 > 1:
            return None
        q = _cross(t, e0)
        t1 = F32(_dot(rd, q) * inv_det)
        if t1 < 0 or t1 > 1:
            return None
        t_cam = F32(_dot(e1, q) * inv_det)
        if t_cam <= Q.TNEAR or t_cam >= tfar:
            return None
        return t_cam, F32(t0 * pl.l0), F32(t1 * pl.l1)


def _plane_contribute(pl, medium, visible, ro, rd, its):
    t_cam, t0, _ = its
    p_its = (ro + rd * t_cam).astype(np.float32)
    p0 = (pl.o + pl.d0 * t0).astype(np.float32)
    if not visible(p0, p_its):
        return None
    sigma_t = (np.asarray(medium.sigma_a, np.float32) + np.asarray(medium.sigma_s, np.float32)) * F32(1.0)
    sigma_s = np.asarray(medium.sigma_s, np.float32)
    transmittance = B._expf(-_color_times(sigma_t, t_cam))
    phase_func = np.full(3, F32(1.0) / (F32(np.pi) * F32(4.0)), np.float32)
    with np.errstate(all="ignore"):
        inv_jacobian = F32(F32(1.0) / abs(_dot(pl.d0, _cross(pl.d1, -rd))))
    return _color_times(((((pl.weight * phase_func) * sigma_s) * sigma_s) * transmittance).astype(np.float32), inv_jacobian)


def _scalar_plane_gather(tree, planes, medium, norm, visible, ro, rd, tfar, c):
    counts = [0, 0]
    stack = [] if tree["root"] is None else [tree["root"]]
    while stack:
        node = tree["nodes"][stack.pop()]
        if not B._box_entered(node["lo"], node["hi"], ro[None, :], rd[None, :], np.asarray([tfar], np.float32))[0]:
            continue
        if node["left"] is None and node["right"] is None:
            for place in range(node["first"], node["first"] + node["count"]):
                pl = planes[int(tree["order"][place])]
                its = _plane_its(pl, ro, rd, tfar)
                if its is None:
                    continue
                counts[0] += 1
                val = _plane_contribute(pl, medium, visible, ro, rd, its)
                if val is not None:
                    counts[1] += 1
                    c = c + _color_times(val, norm)
        else:
            if node["left"] is not None:
                stack.append(node["left"])
            if node["right"] is not None:
                stack.append(node["right"])
    return c, counts


def _random_planes(rs, n):
    def dirs():
        d = rs.normal(size=(n, 3))
        return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return Q.plane_words(rs.uniform(-1, 1, (n, 3)), dirs(), dirs(), rs.uniform(0.2, 2.0, n), rs.uniform(0.2, 2.0, n), rs.uniform(0.1, 3.0, (n, 3)), np.arange(n), 1)


class _Half:
    """A stand-in scene for the restatement's visibility: a wall at x = 0.25 that hides a segment crossing it."""
    @staticmethod
    def visible(p0, p1):
        p0, p1 = np.asarray(p0, np.float32).reshape(-1, 3), np.asarray(p1, np.float32).reshape(-1, 3)
        return ((p0[:, 0] < 0.25) == (p1[:, 0] < 0.25)).astype(np.uint8)


@pytest.mark.parametrize("seed,sigma_a,sigma_s", [(1, (0.0,) * 3, (1.0,) * 3), (2, (0.1, 0.2, 0.3), (0.9, 0.4, 0.0))])
def test_two_tree_gather_equals_the_scalar_walk(built, seed, sigma_a, sigma_s):
    rs = np.random.RandomState(seed)
    beam_words, plane_words = _random_beams(rs, 10, zero_every=5), _random_planes(rs, 23)
    medium = _medium(sigma_a, sigma_s)
    radius, n_paths = 0.4, 7
    ro, rd, tfar = _random_rays(rs, 120)
    sub = R.split(beam_words)
    beam_tree = R.build_tree(sub, radius)
    beams = R.Beams(sub, n_paths, radius, medium)
    planes = Q.Planes(_Half, plane_words, n_paths, medium)
    plane_tree = P.build_tree(planes.planes)
    c, _, accepted, _ = R.gather(beam_tree, beams, ro, rd, tfar)
    counts, _ = Q.gather_planes(plane_tree, planes, ro, rd, tfar, c)
    total = [0, 0, 0]
    for k in range(ro.shape[0]):
        want, n = _scalar_gather(beam_tree, sub, radius, medium, beams.norm, ro[k], rd[k], tfar[k])      # c = 0; the beams ...
        want, (isect, vis) = _scalar_plane_gather(plane_tree, planes.planes, medium, planes.norm, lambda a, b: bool(_Half.visible(a, b)[0]), ro[k], rd[k], tfar[k], want)
        np.testing.assert_array_equal(c[k].view(np.uint32), want.view(np.uint32), err_msg=f"ray {k}")       # ... then the planes, into the same c
        total = [total[0] + n, total[1] + isect, total[2] + vis]
    assert total == [accepted, counts[1], counts[2]] and accepted >= 10 and counts[2] >= 20 and counts[1] > counts[2]


def test_closed_form_of_one_unit_square_plane(built):
    """The plane o = (0, 0, 2), d0 = x, d1 = y, both lengths 1, and a camera ray from the origin through its interior: t_cam = 2 / d.z, and the contribution is
    radiance * sigma_s^2 * exp(-sigma_t t) / (4 pi |d0 . (d1 x -d)|) / n_paths with |d0 . (d1 x -d)| = |d.z|."""
    medium = _medium((0.25,) * 3, (0.5,) * 3)
    rad = (1.0, 2.0, 4.0)
    n_paths = 5
    always = types.SimpleNamespace(visible=lambda a, b: np.ones(np.asarray(a).reshape(-1, 3).shape[0], np.uint8))
    planes = Q.Planes(always, Q.plane_words([(0.0, 0.0, 2.0)], [(1.0, 0.0, 0.0)], [(0.0, 1.0, 0.0)], 1.0, 1.0, [rad]), n_paths, medium)
    ro = np.zeros((1, 3), np.float32)
    tfar = np.asarray([10.0], np.float32)

    def through(x, y, tf=tfar, pl=planes):
        d = np.asarray([[x, y, 2.0]], np.float64)
        d = (d / np.linalg.norm(d)).astype(np.float32)
        ok, vis, val = pl.hits(0, ro, d, tf)
        return d[0], ok[0], val

    d, ok, val = through(0.3, 0.6)
    assert ok
    t = 2.0 / float(d[2])
    want = np.asarray(rad) * 0.5 * 0.5 * math.exp(-0.75 * t) / (4 * math.pi * abs(float(d[2]))) / n_paths
    np.testing.assert_allclose(val[0], want, rtol=4e-6)
    assert not through(-0.01, 0.5)[1] and not through(0.5, -0.01)[1]          # outside: t0 < 0, t1 < 0
    assert not through(1.001, 0.5)[1] and not through(0.5, 1.001)[1]          # t0, t1 just past 1
    assert through(0.999, 0.999)[1]
    assert not through(0.3, 0.6, np.asarray([1.9], np.float32))[1]            # past tfar
    # |det| < 1e-5: a plane seen edge-on (the ray lies in it), and a plane whose area is below the threshold
    edge_on = Q.Planes(always, Q.plane_words([(0.0, 0.0, 2.0)], [(0.0, 0.0, 1.0)], [(0.0, 1.0, 0.0)], 1.0, 1.0, [rad]), n_paths, medium)
    assert not edge_on.hits(0, ro, np.asarray([[0.0, 0.0, 1.0]], np.float32), tfar)[0][0]
    tiny = Q.Planes(always, Q.plane_words([(0.0, 0.0, 2.0)], [(1.0, 0.0, 0.0)], [(0.0, 1.0, 0.0)], 1e-3, 1e-3, [rad]), n_paths, medium)
    assert not through(0.0005, 0.0005, pl=tiny)[1]
    # hidden: the contribution is black and the plane still counts as intersected
    never = types.SimpleNamespace(visible=lambda a, b: np.zeros(np.asarray(a).reshape(-1, 3).shape[0], np.uint8))
    hidden = Q.Planes(never, Q.plane_words([(0.0, 0.0, 2.0)], [(1.0, 0.0, 0.0)], [(0.0, 1.0, 0.0)], 1.0, 1.0, [rad]), n_paths, medium)
    _, ok, val = through(0.3, 0.6, pl=hidden)
    assert ok and val.shape[0] == 0


# ---- the fixtures, and the host's plane tree over the new records
@pytest.fixture(scope="module")
def fixture(built):
    sd = scenes.cbox_medium(32, 24, 1.0)
    return sd, {pp: Q.compute(sd, seed=3, nb_primitive=64, spp=2, radius=0.05, per_path=pp) for pp in (False, True)}


@pytest.mark.parametrize("per_path", [False, True])
def test_fixture_holds_every_kind_of_record(fixture, per_path):
    sd, out = fixture
    gen = out[per_path]["gen"]
    beams, planes = gen["beams"], gen["planes"]
    assert planes.shape[0] >= 64 and gen["n_paths"] >= 5
    surf = (beams[:, 7] & 1) == 1
    assert surf.any() and (~surf).any()                           # beams from the light or a surface, and beams from the medium
    kinds = {"surface": 0, "unexpanded": 0, "long": 0}
    for k, (edges, _) in enumerate(gen["paths"]):
        for j, e in enumerate(edges):
            if e["from_surface"]:
                continue
            if j + 1 == len(edges):
                kinds["unexpanded"] += 1                          # a volume-origin beam whose end vertex was not expanded
            elif edges[j + 1]["from_surface"]:
                kinds["surface"] += 1                             # a volume-origin beam that ends on a surface
            elif edges[j + 1]["ct"] > edges[j + 1]["length"]:
                kinds["long"] += 1                                # a plane whose second edge ended on a surface: length1 > the hit distance
    assert all(v > 0 for v in kinds.values()), kinds
    img = out[per_path]["image"]
    assert np.isfinite(img).all() and (img.sum(axis=2) > 0).mean() >= 0.25
    st = out[per_path]["stats"]
    assert st["beams_accepted"] > 0 and 0 < st["planes_visible"] < st["planes_intersected"]


@pytest.mark.parametrize("per_path", [False, True])
def test_host_plane_tree_over_the_new_records(fixture, per_path):
    sd, out = fixture
    planes = out[per_path]["gen"]["planes"]
    for n in (1, 3, 4, 5, 9, planes.shape[0]):
        words = planes[:n]
        tree = P.build_tree([P.plane_from_words(w) for w in words])
        assert_trees_equal(api.plane_tree_build(words), R.tree_arrays(tree), f"{n} planes")
    sub = api.beam_split(out[per_path]["gen"]["beams"])
    np.testing.assert_array_equal(sub, R.split(out[per_path]["gen"]["beams"]))
    assert_trees_equal(api.beam_tree_build(sub, 0.05), R.tree_arrays(R.build_tree(sub, 0.05)), "beams")


def test_classes(built):
    assert api.PPLANE_RECORD_DTYPE.itemsize == 4 * api.PLANE_WORDS
    with pytest.raises(ValueError):
        api.IntegratorPhotonPlanes(light_streams="other")
    for name in ("rl_pplane_generate", "rl_pplane_generate_paths", "rl_pplane_map_build", "rl_pplane_map_build_words", "rl_render_photon_planes"):
        assert name in api.PUBLIC_SYMBOLS and hasattr(api.lib(), name)
