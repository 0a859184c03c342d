"""tests/pnats_restatement.py held to four things on the CPU: (1) a literal scalar transcription of LightBounds::importance_ray and LightSamplerATS::sample
(emitter.rs:975-1032, 1361-1399; math.rs:5-31, 74-88), float32 operation by operation, on a few hundred random (ray, max_dist | None, node) triples with
the two defined panics, a max_dist shorter than the foot of the perpendicular and a foot behind the origin among them; (2) the walk is a probability; (3)
a cluster that faces away from the whole segment has importance 0 and is not picked while its sibling has importance; (4) the host tree, the oracle's tree
and the side array of angles agree node for node.  Then the two forms of the drivers (the literal walk of a block, the array form with the chain walk)
against each other, and the draw counts."""
import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api
from tests import pn_restatement as P
from tests import pnats_restatement as A
from tests.bre_restatement import F32

ONE, ZERO = F32(1.0), F32(0.0)


# ---- (1) the scalar transcription: np.float32 scalars, one statement of the reference per line
def s_dot(a, b):
    return F32(F32(F32(a[0] * b[0]) + F32(a[1] * b[1])) + F32(a[2] * b[2]))


def s_vec(x, y, z):
    return np.asarray([x, y, z], np.float32)


def s_cross(a, b):
    return s_vec(F32(a[1] * b[2]) - F32(a[2] * b[1]), F32(a[2] * b[0]) - F32(a[0] * b[2]), F32(a[0] * b[1]) - F32(a[1] * b[0]))


def s_normalize(a):
    with np.errstate(all="ignore"):
        inv = F32(ONE / np.sqrt(s_dot(a, a)))
        return s_vec(a[0] * inv, a[1] * inv, a[2] * inv)


def s_max(a, b):
    return F32(np.fmax(F32(a), F32(b)))                                                      # f32::max: the operand that is no NaN


def s_acos_fast(x):
    with np.errstate(all="ignore"):
        x1 = F32(abs(x))
        x2 = F32(x1 * x1)
        x3 = F32(x2 * x1)
        s = F32(F32(F32(-0.2121144) * x1) + F32(np.pi / 2))
        s = F32(F32(F32(0.0742610) * x2) + s)
        s = F32(F32(F32(-0.0187293) * x3) + s)
        s = F32(F32(np.sqrt(F32(ONE - x1))) * s)
        return s if x >= ZERO else F32(F32(np.pi) - s)


def s_importance_ray(tree, i, o, d, max_dist):
    """max_dist: an f32, or None."""
    with np.errstate(all="ignore"):
        bmin, bmax, w = tree.bmin[i], tree.bmax[i], tree.axis[i]
        pc = s_vec(*[F32(F32(F32(bmax[k] - bmin[k]) * F32(0.5)) + bmin[k]) for k in range(3)])
        diff = s_vec(*[F32(pc[k] - o[k]) for k in range(3)])
        t = s_dot(d, diff)
        if t > ZERO:
            if max_dist is not None:
                t = t if max_dist >= t else max_dist
        else:
            t = ZERO
        closest = s_vec(*[F32(o[k] + F32(d[k] * t)) for k in range(3)])
        pcl = s_vec(*[F32(pc[k] - closest[k]) for k in range(3)])
        dist = F32(np.sqrt(s_max(s_dot(pcl, pcl), F32(0.0001))))
        v0 = s_normalize(s_vec(*[F32(o[k] - pc[k]) for k in range(3)]))
        if max_dist is not None:
            v1 = s_normalize(s_vec(*[F32(F32(o[k] + F32(d[k] * max_dist)) - pc[k]) for k in range(3)]))
        else:
            v1 = s_vec(-d[0], -d[1], -d[2])
        up = s_normalize(s_cross(v0, v1))
        o1 = s_cross(up, v0)
        dot_o0, dot_o1 = s_dot(v0, w), s_dot(o1, w)
        length_1 = F32(np.sqrt(s_max(F32(F32(dot_o0 * dot_o0) + F32(dot_o1 * dot_o1)), ZERO)))
        cos_phi_0 = F32(dot_o0 / length_1)
        if not np.isfinite(cos_phi_0):
            return ZERO, True                                                                # the assert: the defined panic
        if dot_o1 < ZERO or s_dot(v0, v1) < cos_phi_0:
            cos_theta_min = s_max(s_dot(v0, w), s_dot(v1, w))
        else:
            sin_phi_0 = F32(np.sqrt(F32(ONE - F32(cos_phi_0 * cos_phi_0))))
            cos_theta_min = s_dot(s_vec(*[F32(F32(v0[k] * cos_phi_0) + F32(o1[k] * sin_phi_0)) for k in range(3)]), w)
        theta_min = s_acos_fast(cos_theta_min)
        # DirectionCone::subtended_directions(aabb, closest)
        radius = F32(np.sqrt(s_dot(*[s_vec(*[F32(pc[k] - bmax[k]) for k in range(3)])] * 2)))
        pcc = s_vec(*[F32(closest[k] - pc[k]) for k in range(3)])
        if s_dot(pcc, pcc) < F32(radius * radius):
            cos_u = F32(-1.0)
        else:
            cos_u = F32(np.sqrt(s_max(F32(ONE - F32(F32(radius * radius) / s_dot(pcl, pcl))), ZERO)))
        theta_u = s_acos_fast(cos_u)
        theta_p = s_max(F32(F32(theta_min - tree.theta_o[i]) - theta_u), ZERO)
        if theta_p >= tree.theta_e[i]:
            return ZERO, False
        cos_p = P._cos(np.asarray([theta_p], np.float32))[0]
        return s_max(F32(F32(tree.phi[i] * cos_p) / dist), ZERO), False


def s_sample(tree, r, importance):
    pdf_sel, node = ONE, tree.root
    with np.errstate(all="ignore"):
        while True:
            if tree.left[node] < 0 and tree.right[node] < 0:
                return int(tree.light[node]), pdf_sel
            imp_left, imp_right = importance(int(tree.left[node])), importance(int(tree.right[node]))
            prob_left = F32(0.5) if imp_left == ZERO and imp_right == ZERO else F32(imp_left / F32(imp_left + imp_right))
            if r < prob_left:
                r = F32(r / prob_left); node = int(tree.left[node]); pdf_sel = F32(pdf_sel * prob_left)
            else:
                r = F32(F32(r - prob_left) / F32(ONE - prob_left)); node = int(tree.right[node]); pdf_sel = F32(pdf_sel * F32(ONE - prob_left))


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v)).astype(np.float32)


def _triples(tree, rng, n):
    """(node, o, d, max_dist | None, kind): random ones, then the four named cases."""
    out = []
    for _ in range(n):
        i = int(rng.integers(tree.n))
        o = np.asarray([rng.uniform(-1, 1), rng.uniform(0, 2), rng.uniform(1, 7)], np.float32)
        d = _unit([rng.normal(0, 0.3), rng.normal(0, 0.3), -1.0]) if rng.random() < 0.8 else _unit(rng.normal(size=3))
        out.append((i, o, d, None if rng.random() < 0.25 else F32(rng.uniform(0.05, 9.0)), "random"))
    leaves = [i for i in range(tree.n) if tree.left[i] < 0]
    for i in range(tree.n):
        pc = tree.centre(i)
        # through the cluster's centre, along an axis of the frame: v0 x v1 = 0 exactly
        out.append((i, (pc + np.asarray([2.0, 0.0, 0.0], np.float32)).astype(np.float32), np.asarray([-1.0, 0.0, 0.0], np.float32), F32(3.0), "through the centre"))
        out.append((i, (pc + np.asarray([0.0, 0.0, 1.5], np.float32)).astype(np.float32), np.asarray([0.0, 0.0, -1.0], np.float32), None, "through the centre"))
        # the foot of the perpendicular lies beyond max_dist, and behind the origin
        o = (pc + np.asarray([0.3, -0.4, 3.0], np.float32)).astype(np.float32)
        out.append((i, o, np.asarray([0.0, 0.0, -1.0], np.float32), F32(1.25), "short"))
        out.append((i, o, np.asarray([0.0, 0.0, 1.0], np.float32), F32(2.0), "behind"))
        out.append((i, o, np.asarray([0.0, 0.0, 1.0], np.float32), None, "behind"))
    for i in leaves:
        if tree.axis[i][0] == 0.0 and tree.axis[i][2] == 0.0:                                # the axis is +-y exactly: a ray in the plane y = centre.y is normal to it
            pc = tree.centre(i)
            o = (pc + np.asarray([0.5, 0.0, 2.0], np.float32)).astype(np.float32)
            o[1] = pc[1]
            out.append((i, o, _unit([0.25, 0.0, -1.0]), F32(3.0), "axis normal to the plane"))
    return out


@pytest.fixture(scope="module")
def lights8(built):
    return A.frame("lights8")


def test_importance_ray_is_the_scalar_transcription(lights8):
    tree = lights8.tree
    rng = np.random.default_rng(11)
    seen = {}
    for i, o, d, max_dist, kind in _triples(tree, rng, 300):
        want, panicked = s_importance_ray(tree, i, o, d, max_dist)
        got = tree.importance_ray(i, o[None, :], d[None, :], np.asarray([max_dist is not None]), np.asarray([0.0 if max_dist is None else max_dist], np.float32))[0]
        assert F32(got).tobytes() == F32(want).tobytes(), (kind, i, o, d, max_dist, got, want)
        seen[kind] = seen.get(kind, 0) + 1
        seen["panic"] = seen.get("panic", 0) + int(panicked)
        seen["positive"] = seen.get("positive", 0) + int(want > 0)
        if kind in ("through the centre", "axis normal to the plane"):
            assert panicked and got == 0.0, (kind, i)
    assert seen["random"] == 300 and seen["through the centre"] == 2 * tree.n and seen["short"] == tree.n and seen["behind"] == 2 * tree.n
    assert seen.get("axis normal to the plane", 0) >= 4 and seen["positive"] >= 100


def test_the_closest_point_clamps_to_the_segment():
    pc = np.asarray([0.0, 0.0, 0.0], np.float32)
    o = np.asarray([[0.3, -0.4, 3.0]] * 3, np.float32)
    d = np.asarray([[0, 0, -1], [0, 0, -1], [0, 0, 1]], np.float32)
    closest, d2 = A.closest_point(o, d, np.asarray([True, False, True]), np.asarray([1.25, 0.0, 2.0], np.float32), pc)
    assert np.array_equal(closest, np.asarray([[0.3, -0.4, 1.75], [0.3, -0.4, 0.0], [0.3, -0.4, 3.0]], np.float32))      # max_dist short of the foot | the foot | the origin
    assert np.allclose(d2, [0.25 + 1.75 ** 2, 0.25, 0.25 + 9.0])


def test_acos_fast_is_the_cubic_not_acos():
    x = np.linspace(-1, 1, 41).astype(np.float32)
    got = A.acos_fast(x)
    assert all(F32(g).tobytes() == F32(s_acos_fast(v)).tobytes() for g, v in zip(got, x))
    err = np.abs(got.astype(np.float64) - np.arccos(x.astype(np.float64)))
    assert 1e-6 < err.max() < 1e-3 and got[0] == F32(np.pi) and got[-1] == 0.0


def test_sample_is_the_scalar_walk(lights8):
    tree = lights8.tree
    rng = np.random.default_rng(5)
    n = 200
    o = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(0.5, 1.5, n), np.full(n, 6.8)], axis=-1).astype(np.float32)
    d = np.stack([_unit([rng.normal(0, 0.15), rng.normal(0, 0.15), -1.0]) for _ in range(n)])
    has_max = rng.random(n) < 0.8
    max_dist = rng.uniform(4.0, 8.0, n).astype(np.float32)
    r = rng.random(n).astype(np.float32)
    light, pdf = tree.sample(r, lambda node, m: tree.importance_ray(node, o[m], d[m], has_max[m], max_dist[m]))
    for k in range(n):
        want = s_sample(tree, r[k], lambda node: s_importance_ray(tree, node, o[k], d[k], max_dist[k] if has_max[k] else None)[0])
        assert (int(light[k]), F32(pdf[k]).tobytes()) == (want[0], F32(want[1]).tobytes()), k
    assert len(set(light.tolist())) >= 8, "the walks end at many leaves"
    # the point arm: the same walk with importance_point
    p = np.stack([rng.uniform(-0.9, 0.9, n), rng.uniform(0.1, 1.9, n), rng.uniform(-0.9, 0.9, n)], axis=-1).astype(np.float32)
    light, pdf = tree.sample(r, lambda node, m: tree.importance_point(node, p[m]))
    for k in range(0, n, 4):
        want = s_sample(tree, r[k], lambda node: tree.importance_point(node, p[k:k + 1])[0])
        assert (int(light[k]), F32(pdf[k]).tobytes()) == (want[0], F32(want[1]).tobytes()), k


def test_importance_point_is_the_oracles(lights8):
    """The point arm's importance against the oracle's importance_point (orc_ats_probe, which the device's ats_importance is held to): through the walk's
    probabilities, which the oracle reports for a point without a normal."""
    tree, sc = lights8.tree, lights8.sc
    mesh_of = [k for k, m in enumerate(lights8.sd.meshes) if m.emission is not None]
    rng = np.random.default_rng(3)
    for _ in range(40):
        p = np.asarray([rng.uniform(-0.9, 0.9), rng.uniform(0.1, 1.9), rng.uniform(-0.9, 0.9)], np.float32)
        r = F32(rng.random())
        light, pdf = tree.sample(np.asarray([r]), lambda node, m: tree.importance_point(node, p[None, :][m]))
        got = sc.sample_light(p, float(r), 0.5, 0.25, 0.75)
        assert got["emitter"] == mesh_of[int(tree.light_emitter[light[0]])], (p, r)
        pos, nrm, _, _ = lights8.pick.at_point(p[None, :], np.asarray([r]), np.asarray([0.25], np.float32), np.asarray([0.75], np.float32))
        assert pos[0].tobytes() == got["p"].tobytes() and nrm[0].tobytes() == got["n"].tobytes()      # the same triangle of it, the same point


# ---- (2) the walk is a probability
def test_the_walk_is_a_probability(lights8):
    tree = lights8.tree
    rng = np.random.default_rng(17)
    for k in range(40):
        o = np.asarray([[rng.uniform(-0.5, 0.5), rng.uniform(0.5, 1.5), 6.8]], np.float32)
        d = _unit([rng.normal(0, 0.15), rng.normal(0, 0.15), -1.0])[None, :]
        has_max, max_dist = np.asarray([k % 5 != 0]), np.asarray([rng.uniform(4.0, 8.0)], np.float32)
        imp = lambda node, m=None: tree.importance_ray(node, o, d, has_max, max_dist)
        probs = tree.leaf_probabilities(imp)
        assert len(probs) == 16 and abs(sum(float(v) for v in probs.values()) - 1.0) <= 16 * 5 * 2.0 ** -23      # 16 leaves, depth 5, one rounding per product
        for r in rng.random(8).astype(np.float32):
            light, pdf = tree.sample(np.asarray([r]), imp)
            assert F32(pdf[0]).tobytes() == F32(probs[int(light[0])]).tobytes()


# ---- (3) a cluster that faces away
def test_a_light_that_faces_away_from_the_segment_is_not_picked(lights8):
    """The quad in front of the back wall emits towards -z from z = -0.7.  A camera ray that ends at z = 0.5 has no point in front of it, and none within
    the angle the proxy's bounding sphere adds to the cone (the importance is a bound: a segment that ends 0.1 behind the quad's plane still gets some): both
    its proxies have importance 0, and the walk does not reach them wherever their sibling has importance.
    This holds where the reference measures the angle at the segment's ends (dot_o1 < 0, found here in float64 from the geometry alone).  Where dot_o1 >= 0
    its test `v0 . v1 < cos_phi_0` sends a cluster whose phi_0 lies far outside the arc (cos_phi_0 near -1) to the in-plane branch, cos_theta_min is the
    length of the axis' projection, and the light that faces away gets importance: an overestimate, kept as the reference has it, and asserted present."""
    tree, sd = lights8.tree, lights8.sd
    emissive = [m for m in sd.meshes if m.emission is not None]
    e_back = [k for k, m in enumerate(emissive) if m.name == "L4"][0]
    back = [int(i) for i in range(tree.n) if tree.left[i] < 0 and tree.light_emitter[tree.light[i]] == e_back]
    assert len(back) == 2 and all(tree.axis[i][2] < -0.99 for i in back)
    rng = np.random.default_rng(23)
    n = 64
    o = np.tile(np.asarray([[0.0, 1.0, 6.8]], np.float32), (n, 1))
    d = np.stack([_unit([rng.normal(0, 0.12), rng.normal(0, 0.12), -1.0]) for _ in range(n)])
    has_max = np.ones(n, bool)
    max_dist = ((6.8 - 0.5) / -d[:, 2]).astype(np.float32)                                    # the segment ends at z = 0.5
    ends = np.ones(n, bool)
    for i in back:
        pc = tree.centre(i).astype(np.float64)
        v0 = o.astype(np.float64) - pc
        v1 = o.astype(np.float64) + d.astype(np.float64) * max_dist[:, None].astype(np.float64) - pc
        o1 = np.cross(np.cross(v0, v1), v0)
        ends &= (o1 @ tree.axis[i].astype(np.float64)) / np.linalg.norm(o1, axis=1) < -1e-3
    assert 0.25 <= ends.mean() <= 0.75
    for i in back:
        imp = tree.importance_ray(i, o, d, has_max, max_dist)
        assert not imp[ends].any() and imp[~ends].any()
    o, d, has_max, max_dist, n = o[ends], d[ends], has_max[ends], max_dist[ends], int(ends.sum())
    guarded = 0
    for k in range(n):
        imp = lambda node, m=None: tree.importance_ray(node, o[k:k + 1], d[k:k + 1], has_max[k:k + 1], max_dist[k:k + 1])
        probs = tree.leaf_probabilities(imp)
        pair = int(tree.parent[back[0]])                                                     # the quad's two triangles are siblings: their cluster faces away too
        assert pair == int(tree.parent[back[1]]) and imp(pair)[0] == 0.0
        above = int(tree.parent[pair])
        sibling = int(tree.right[above]) if int(tree.left[above]) == pair else int(tree.left[above])
        if imp(sibling)[0] > 0:
            guarded += 1
            assert all(probs[int(tree.light[i])] == 0.0 for i in back)
    assert guarded >= n // 2
    light, _ = tree.sample(rng.random(n).astype(np.float32), lambda node, m: tree.importance_ray(node, o[m], d[m], has_max[m], max_dist[m]))
    assert not np.isin(light, [int(tree.light[i]) for i in back]).any()


# ---- (4) the three trees
@pytest.mark.parametrize("name", ["box", "lights8", "lights8_hg", "two_lights"])
def test_host_tree_oracle_tree_and_angles_agree(built, name):
    sd = A.scene(name)
    host = api.Scene(sd)
    hn, he, hp = host.debug_ats()
    on, oe, op = orc.Scene(sd).ats_dump()
    assert hn.view(np.uint32).tobytes() == on.view(np.uint32).tobytes() and np.array_equal(he, oe) and np.array_equal(hp, op)
    angles = host.debug_ats_angles()
    assert angles.shape == (hn.shape[0], 2) and angles.dtype == np.float32
    tree = A.Tree(on, oe, op, angles)
    # the stored cosines are the cosines of the stored angles (LightBounds::union: cos_theta_o = theta_o.cos())
    assert P._cos(angles[:, 0]).tobytes() == tree.cos_o.tobytes() and P._cos(angles[:, 1]).tobytes() == tree.cos_e.tobytes()
    for i in range(tree.n):
        if tree.left[i] < 0:
            assert angles[i, 0] == 0.0 and angles[i, 1] == F32(np.pi / 2)                    # convert_light_proxy
        else:
            assert angles[i, 1] == max(angles[tree.left[i], 1], angles[tree.right[i], 1]) and 0.0 <= angles[i, 0] <= F32(np.pi)
    assert api.Scene(P.scene("box")).debug_ats_angles().shape == (0, 2)                      # no tree, no angles


# ---- the drivers
def test_draw_counts():
    assert [A.draws_per_sample(s, False) for s in api.PN_STRATEGIES] == [4, 3, 4, 6, None, None, None]
    assert [A.draws_per_sample(s) for s in api.PN_STRATEGIES] == [6, 5, 6, 8, None, None, None]
    assert all(A.draws_per_sample(s) is None for s in api.PN_TAYLOR_STRATEGIES)
    # one less than over the power pick, but for tr_phase, which has no emitter sample
    assert [P.draws_per_sample(s) - A.draws_per_sample(s) for s in ("tr_ex", "tr_phase", "eq_ex", "eq_phase")] == [1, 0, 1, 1]


@pytest.mark.parametrize("strategy", ["tr_ex", "eq_phase", "eq_clamped_ex", "eq_clamped_phase", "pn_ex", "eq_tr_taylor_ex", "pn_tr_taylor_ex"])
def test_the_block_walk_and_the_array_form_agree(built, strategy):
    """The literal loop over a block, every draw taken where the reference takes it (the walk asserts its count against the body's), against the array form
    with its jump or its chain walk: image, counters and where every pixel starts in the block's stream."""
    fr = A.frame("lights8", 12, 7)
    seeds = orc.block_seeds(3, 12, 7)
    for mode in (api.STREAM_REFERENCE_ORDER, api.STREAM_PER_SAMPLE):
        a = A.render(fr, seeds, strategy, 2, True, mode)
        b = A.render_walk(fr, seeds, strategy, 2, True, mode)
        assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and (a[0].any() or P.is_phase(strategy))
        if mode == api.STREAM_REFERENCE_ORDER:
            assert all(np.array_equal(a[2]["starts"][k], b[2]["starts"][k]) for k in a[2]["starts"])
        if strategy in ("pn_ex", "pn_tr_taylor_ex") and mode == api.STREAM_REFERENCE_ORDER:      # (the clamped samplers are None for a few rays in a thousand)
            assert a[2]["none"] > 0 and a[2]["some"] > 0


def test_tr_phase_is_the_plain_restatement_without_the_tree(built):
    sd = A.lights(8, 12, 7, hsv=False)
    seeds = orc.block_seeds(3, 12, 7)
    plain = A.lights(8, 12, 7, hsv=False, use_ats=False)
    a = A.render(A.Frame(sd), seeds, "tr_phase", 4)
    b = P.render(P.Frame(plain), seeds, "tr_phase", 4)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]


def test_refusals():
    for kw in ({"use_ats": False}, {}):
        sd = A.lights(2, 8, 8, **kw)
        if not kw:
            sd.lights.append(dict(P.POINT_LIGHT))
        with pytest.raises(A.Refused) as e:
            A.check_scene(sd)
        assert e.value.code == api.RL_ERR_UNSUPPORTED
    with pytest.raises(A.Refused) as e:
        A.check_params("eq_best_ex", 1, api.STREAM_REFERENCE_ORDER, 0, 1)
    assert e.value.code == P.RL_ERR_INVALID_ARGUMENT
