"""IntegratorSinglePlane restated in float32 numpy from the reference's text, the yardstick of tests/test_plane_single_restatement.py and
tests/test_gpu_plane_single_exact.py (a plain module: `from tests import plane_single_restatement`).

What is restated (src/integrators/explicit/plane_single.rs unless another file is named): RectangularLightSource::from_shape (38-75), the plane pass
(326-427) with cosine_sample_hemisphere / concentric_sample_disk and Frame (src/math.rs:37-65, 357-375) and HomogenousVolume::sample's continued_t
(src/volume.rs:95-135), SinglePhotonPlane::new / aabb / position / intersection / light_position / contrib (101-277), BHVAccel::create and gather
(src/accel.rs:458-581), the weights and fluxes of the seven strategies and the camera loop (436-611), Color's guarded operators (src/structure.rs:249-303).
What is taken from the oracle's existing entry points: orc.Rng, the block seeds, camera_generate and trace (through bre_restatement.camera_samples), visible,
and orc_math_batch for sin, cos, exp and log.

Every float operation is a float32 scalar or elementwise numpy operation in the reference's order (dot = (x x' + y y') + z z', nothing fused, powi(2) as
x * x, powi(-1) as 1 / x); f32::max / min are np.fmax / np.fmin.  The generation is scalar; the gather is vectorised over the camera samples exactly as
tests/bre_restatement.py vectorises its walk.  The stated differences from the reference: the sort is stable, and id_emitter is clamped to the last light."""

import numpy as np

from oracle import orc
from rustlight_amd import abi, api
from tests.bre_restatement import F32, F32_MAX, TNEAR, _box_entered, _expf, _scale, camera_samples, visit_order

PI, FRAC_PI_2, FRAC_PI_4 = F32(np.pi), F32(np.pi / 2), F32(np.pi / 4)
ONE, ZERO = F32(1.0), F32(0.0)
UV, VT, UT, UALPHAT = api.PLANE_UV, api.PLANE_VT, api.PLANE_UT, api.PLANE_UALPHAT
STRATEGIES = api.PLANE_STRATEGIES
# The plane counts of the image fixtures (cbox_medium(32, 24, 1.0), seed 3, spp 2): 64, raised for the two strategies whose image at 64 planes is non-zero in
# fewer than a quarter of the pixels (uv: 69 of 768 at 64, 160 at 256, 218 at 512; vt: 134 at 64, 208 at 256) — tests/test_plane_single_restatement.py
# asserts the quarter of every one before anything is compared with them
FIXTURE_NB = {"uv": 512, "vt": 256, "ut": 64, "average": 64, "discrete_mis": 64, "ualpha": 64, "cmis": 64}


# ---- the float32 pieces
def _math(fn, x):
    a = np.ascontiguousarray(x, np.float32).reshape(-1)
    out = np.zeros_like(a)
    if a.size:
        orc.lib().orc_math_batch(fn, a.size, abi.fptr(a), abi.fptr(a), abi.fptr(out))
    return out.reshape(np.shape(x)) if np.ndim(x) else F32(out[0])


def _sin(x):
    return _math(0, x)


def _cos(x):
    return _math(1, x)


def _ln(x):
    return _math(3, x)


def _v(x):
    return np.asarray(x, np.float32)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1).astype(np.float32)


def _mag(a):
    return np.sqrt(_dot(a, a)).astype(np.float32)


def _div_guarded(c, s):
    """Color / f32 (structure.rs:249-265): a zero or non-finite divisor gives black.  c [.., 3], s scalar or [..]."""
    s = _v(s)
    bad = (s == ZERO) | ~np.isfinite(s)
    with np.errstate(all="ignore"):
        return np.where(bad[..., None], ZERO, c / s[..., None]).astype(np.float32)


def _avg(c):
    return ((c[..., 0] + c[..., 1] + c[..., 2]) / F32(3.0)).astype(np.float32)


# ---- RectangularLightSource::from_shape (38-75)
class Light:
    pass


def from_shape(mesh):
    v = _v(mesh.vertices).reshape(-1, 3)
    assert np.asarray(mesh.indices).reshape(-1, 3).shape[0] == 2 and v.shape[0] >= 4 and mesh.emission_kind is None
    l = Light()
    l.o = v[0]
    u, w = v[1] - v[0], v[3] - v[0]
    l.u_l, l.v_l = _mag(u), _mag(w)
    l.u, l.v = u / l.u_l, w / l.v_l
    l.n = _cross(l.u, l.v)
    l.emission = _v(mesh.emission)
    return l


def rect_lights(sd):
    return [from_shape(m) for m in sd.meshes if m.emission is not None]


# ---- src/math.rs:37-65, 357-375
def concentric_sample_disk(ux, uy):
    ox, oy = F32(ux) * F32(2.0) - ONE, F32(uy) * F32(2.0) - ONE
    if ox == ZERO and oy == ZERO:
        return ZERO, ZERO
    if abs(ox) > abs(oy):
        r, theta = ox, FRAC_PI_4 * (oy / ox)
    else:
        r, theta = oy, FRAC_PI_2 - FRAC_PI_4 * (ox / oy)
    return _cos(theta) * r, _sin(theta) * r


def cosine_sample_hemisphere(ux, uy):
    dx, dy = concentric_sample_disk(ux, uy)
    z = np.sqrt(np.fmax(ZERO, ONE - dx * dx - dy * dy))
    return _v([dx, dy, z])


def frame_to_world(n, v):
    sign = F32(np.copysign(1.0, n[2]))
    a = F32(-1.0) / (sign + n[2])
    b = n[0] * n[1] * a
    fx = _v([ONE + sign * n[0] * n[0] * a, sign * b, -sign * n[0]])
    fy = _v([b, sign + n[1] * n[1] * a, -n[1]])
    return ((fx * v[0] + fy * v[1]) + n * v[2]).astype(np.float32)


# ---- SinglePhotonPlane (78-277)
class Plane:
    def words(self):
        w = np.zeros(api.PLANE_WORDS, np.uint32)
        w[:14] = np.concatenate([self.o, self.d0, self.d1, [self.l0, self.l1], self.weight]).astype(np.float32).view(np.uint32)
        w[14:16] = _v(self.sample).view(np.uint32)
        w[16], w[17] = self.type, self.id_emitter
        return w

    def corners(self):
        p0 = self.o + self.d0 * self.l0
        p1 = self.o + self.d1 * self.l1
        p2 = p0 + self.d1 * self.l1
        return _v([self.o, p0, p1, p2])

    def aabb(self):
        lo, hi = np.full(3, F32_MAX, np.float32), np.full(3, -F32_MAX, np.float32)
        for c in self.corners():
            lo, hi = np.fmin(lo, c), np.fmax(hi, c)
        return lo, hi

    def position(self):
        return (self.o + self.d0 * self.l0 * F32(0.5) + self.d1 * self.l1 * F32(0.5)).astype(np.float32)


def plane_from_words(w):
    w = np.ascontiguousarray(w, np.uint32)
    f = w.view(np.float32)
    p = Plane()
    p.o, p.d0, p.d1, p.l0, p.l1, p.weight, p.sample = f[0:3].copy(), f[3:6].copy(), f[6:9].copy(), F32(f[9]), F32(f[10]), f[11:14].copy(), f[14:16].copy()
    p.type, p.id_emitter = int(w[16]), int(w[17])
    return p


def plane_new(t, light, d, sample, sample_alpha, t_sampled, id_emitter, sigma_s):
    p = Plane()
    p.type, p.id_emitter, p.sample = t, id_emitter, _v(sample)
    sx, sy = F32(sample[0]), F32(sample[1])
    t_sampled = F32(t_sampled)
    with np.errstate(all="ignore"):
        if t == UV:
            p.o = light.o + d * t_sampled
            p.d0, p.d1, p.l0, p.l1 = light.u, light.v, light.u_l, light.v_l
            p.weight = (PI * light.emission) / sigma_s
        elif t == VT:
            p.o = light.o + light.u * light.u_l * sx
            p.d0, p.d1, p.l0, p.l1 = light.v, d, light.v_l, t_sampled
            p.weight = (PI * light.u_l) * light.emission
        elif t == UT:
            p.o = light.o + light.v * light.v_l * sy
            p.d0, p.d1, p.l0, p.l1 = light.u, d, light.u_l, t_sampled
            p.weight = (PI * light.v_l) * light.emission
        else:
            alpha = PI * F32(sample_alpha)
            o2 = _v([sx * light.u_l, sy * light.v_l])
            d2 = _v([_cos(alpha), _sin(alpha)])

            def plane2d_its(dd):
                t_0 = (-o2) / dd
                t_1 = (_v([light.u_l, light.v_l]) - o2) / dd
                t_max = np.fmax(t_0, t_1)
                return o2 + dd * np.fmin(t_max[0], t_max[1])

            p1_2d, p2_2d = plane2d_its(d2), plane2d_its(-d2)
            p1 = light.o + p1_2d[0] * light.u + p1_2d[1] * light.v
            p2 = light.o + p2_2d[0] * light.u + p2_2d[1] * light.v
            u_plane = p2 - p1
            length = _mag(u_plane)
            p.o, p.d0, p.d1, p.l0, p.l1 = p1, u_plane / length, d, length, t_sampled
            p.weight = _div_guarded(_scale(PI * light.emission, light.u_l * light.v_l), length)
    for k in ("o", "d0", "d1", "weight"):
        setattr(p, k, _v(getattr(p, k)))
    p.l0, p.l1 = F32(p.l0), F32(p.l1)
    return p


def sigma_t_of(medium):
    return (_v(medium.sigma_a) + _v(medium.sigma_s)) * ONE


# ---- the plane pass (326-427)
def generate(sd, state, nb_primitive, strategy):
    """(planes, words [n, PLANE_WORDS] u32, number_plane_gen, sampler state after [4] u64, draws, redraws of the hemisphere direction)."""
    lights = rect_lights(sd)
    sigma_s, sigma_t = _v(sd.medium.sigma_s), sigma_t_of(sd.medium)
    rng = orc.Rng.from_state([int(v) for v in state])
    planes, n_gen, count = [], 0, {"draws": 0, "redraws": 0}

    def nxt():
        count["draws"] += 1
        return F32(rng.next_f32())

    def generate_plane(t, id_emitter):
        light = lights[id_emitter]
        d_out = cosine_sample_hemisphere(nxt(), nxt())
        while d_out[2] == ZERO:
            count["redraws"] += 1
            d_out = cosine_sample_hemisphere(nxt(), nxt())
        d = frame_to_world(light.n, d_out)
        u = nxt()                                            # m.sample(&ray_med, sampler.next()): continued_t
        component = int(u * F32(3.0))
        u = u * F32(3.0) - F32(component)
        with np.errstate(all="ignore"):
            t_sampled = -_ln(ONE - u) / sigma_t[min(component, 2)]
        sample = (nxt(), nxt())
        return plane_new(t, light, d, sample, nxt(), t_sampled, id_emitter, sigma_s)

    while len(planes) < nb_primitive:
        id_emitter = min(int(nxt() * F32(len(lights))), len(lights) - 1)
        if strategy in ("average", "discrete_mis"):
            kinds = (UV, VT, UT)
        else:
            kinds = ({"uv": UV, "vt": VT, "ut": UT, "ualpha": UALPHAT, "cmis": UALPHAT}[strategy],)
        for t in kinds:
            planes.append(generate_plane(t, id_emitter))
        n_gen += 1
    words = np.stack([p.words() for p in planes])
    return planes, words, n_gen, np.array(list(rng.state), np.uint64), count["draws"], count["redraws"]


# ---- BHVAccel::create / build (accel.rs:458-543) over SinglePhotonPlane::aabb / position
def build_tree(planes):
    """The tree in the form tests/bre_restatement.py gives its photon tree: {"nodes", "root", "order"}."""
    boxes = [p.aabb() for p in planes]
    keys = np.asarray([p.position() for p in planes], np.float32).reshape(-1, 3)
    assert all(np.isfinite(p.corners()).all() for p in planes)
    order = list(range(len(planes)))
    nodes = []

    def build(begin, end):
        if end == begin:
            return None
        lo, hi = np.full(3, F32_MAX, np.float32), np.full(3, -F32_MAX, np.float32)
        for i in range(begin, end):
            lo, hi = np.fmin(lo, boxes[order[i]][0]), np.fmax(hi, boxes[order[i]][1])
        if end - begin <= 4:
            nodes.append({"lo": lo, "hi": hi, "first": begin, "count": end - begin, "left": None, "right": None})
            return len(nodes) - 1
        size = hi - lo
        axis = (0 if size[0] > size[2] else 2) if size[0] > size[1] else (1 if size[1] > size[2] else 2)
        seg = order[begin:end]
        seg.sort(key=lambda i: float(keys[i, axis]))      # stable; -0.0 == +0.0
        order[begin:end] = seg
        split = (begin + end) // 2
        left = build(begin, split)
        right = build(split, end)
        nodes.append({"lo": lo, "hi": hi, "first": 0, "count": 0, "left": left, "right": right})
        return len(nodes) - 1

    root = build(0, len(order))
    return {"nodes": nodes, "root": root, "order": np.asarray(order, np.uint32)}


def sort_keys_distinct(planes):
    keys = np.asarray([p.position() for p in planes], np.float32)
    return all(np.unique(keys[:, a]).shape[0] == keys.shape[0] for a in range(3))


# ---- intersection (121-160), light_position (163-172), contrib (173-176), the weights (486-587)
def intersect(pl, o, d, tfar):
    """(accepted mask, t_cam, t0, t1) of plane pl on rays (o, d, tnear = EPSILON, tfar); the reference's comparisons, so a NaN passes where it passes there."""
    with np.errstate(all="ignore"):
        e0, e1 = pl.d0 * pl.l0, pl.d1 * pl.l1
        p = _cross(d, e1[None, :])
        det = _dot(e0[None, :], p)
        ok = ~(np.abs(det) < F32(1e-5))
        inv_det = ONE / det
        t = (o - pl.o[None, :]).astype(np.float32)
        t0 = _dot(t, p) * inv_det
        ok &= ~((t0 < ZERO) | (t0 > ONE))
        q = _cross(t, e0[None, :])
        t1 = _dot(d, q) * inv_det
        ok &= ~((t1 < ZERO) | (t1 > ONE))
        t_cam = _dot(e1[None, :], q) * inv_det
        ok &= ~((t_cam <= TNEAR) | (t_cam >= tfar))
        return ok, t_cam.astype(np.float32), (t0 * pl.l0).astype(np.float32), (t1 * pl.l1).astype(np.float32)


def light_position(pl, light, t0, t1):
    if pl.type == UV:
        return (light.o[None, :] + light.u[None, :] * t0[:, None] + light.v[None, :] * t1[:, None]).astype(np.float32)
    return (pl.o[None, :] + pl.d0[None, :] * t0[:, None]).astype(np.float32)


def contrib(weight, d0, d1, d):
    """SinglePhotonPlane::contrib for rays d [k, 3]; d0 / d1 are [3] or [k, 3]."""
    d0, d1 = np.broadcast_to(d0, d.shape), np.broadcast_to(d1, d.shape)
    jacobian = np.abs(_dot(_cross(d1, d0), d))
    return _div_guarded(np.broadcast_to(weight, d.shape), jacobian)


def discrete_mis_weights(pl, light, sigma_s, p_hit, p_light, rd):
    """DiscreteMIS's w for the plane's own type, [k] f32."""
    with np.errstate(all="ignore"):
        d = (p_hit - p_light).astype(np.float32)
        t_sampled = _mag(d)
        d = (d / t_sampled[:, None]).astype(np.float32)
        c = {UV: _avg(contrib((PI * light.emission) / sigma_s, light.u, light.v, rd)),          # planes = [UV, UT, VT]
             UT: _avg(contrib((PI * light.v_l) * light.emission, light.u, d, rd)),
             VT: _avg(contrib((PI * light.u_l) * light.emission, light.v, d, rd))}
        inv = [np.where((c[k] != ZERO) & np.isfinite(c[k]), ONE / c[k], ZERO).astype(np.float32) for k in (UV, UT, VT)]
        w = (ONE / c[pl.type]) / ((inv[0] + inv[1]) + inv[2])
        return np.where(np.isfinite(w), w, ZERO).astype(np.float32)


def w_cmis(pl, light, rd):
    with np.errstate(all="ignore"):
        a = _dot(_cross(light.u, pl.d1)[None, :], rd)
        b = _dot(_cross(light.v, pl.d1)[None, :], rd)
        return (ONE / ((F32(2.0) / PI) * np.sqrt(a * a + b * b))).astype(np.float32)


class Gatherer:
    """What the camera loop holds: the planes, the lights, the medium, the strategy and number_plane_gen."""

    def __init__(self, sc, sd, planes, n_gen, strategy):
        self.sc, self.planes, self.strategy = sc, planes, strategy
        self.lights = rect_lights(sd)
        self.sigma_s, self.sigma_t = _v(sd.medium.sigma_s), sigma_t_of(sd.medium)
        self.n_lights = F32(len(self.lights))                          # emitters.len() as f32
        self.inv_gen = ONE / F32(n_gen)                                # 1.0 / number_plane_gen as f32
        self.rho = ONE / (PI * F32(4.0))                               # PhaseFunction::Isotropic(), hard-coded (440)

    def hits(self, p, o, d, tfar):
        """Plane p on the rays: (accepted mask, of those visible mask, contributions [visible, 3])."""
        pl = self.planes[p]
        light = self.lights[pl.id_emitter]
        ok, t_cam, t0, t1 = intersect(pl, o, d, tfar)
        if not ok.any():
            return ok, np.zeros(0, bool), np.zeros((0, 3), np.float32)
        o, d, t_cam, t0, t1 = o[ok], d[ok], t_cam[ok], t0[ok], t1[ok]
        p_hit = (o + d * t_cam[:, None]).astype(np.float32)
        p_light = light_position(pl, light, t0, t1)
        vis = self.sc.visible(p_hit, p_light).astype(bool)
        d, t_cam, p_hit, p_light = d[vis], t_cam[vis], p_hit[vis], p_light[vis]
        tau = np.where(np.isfinite(t_cam)[:, None], self.sigma_t[None, :] * t_cam[:, None], ZERO).astype(np.float32)      # sigma_t * r.tfar (Color * f32)
        trans = _expf(-tau)
        if self.strategy == "average":
            w = np.full(d.shape[0], ONE / F32(3.0), np.float32)
        elif self.strategy == "discrete_mis":
            w = discrete_mis_weights(pl, light, self.sigma_s, p_hit, p_light, d)
        else:
            w = np.ones(d.shape[0], np.float32)
        if self.strategy == "cmis":
            flux = w_cmis(pl, light, d)[:, None] * pl.weight[None, :]
        else:
            flux = contrib(pl.weight, pl.d0, pl.d1, d)
        with np.errstate(all="ignore"):
            c = ((((w * self.rho)[:, None] * trans) * self.sigma_s[None, :]) * flux).astype(np.float32)
        return ok, vis, _scale(_scale(c, self.n_lights), self.inv_gen)


# ---- BHVAccel::gather (accel.rs:545-581) and the sum of plane_single.rs:463-596, over all rays at once
def gather(tree, g, o, d, tfar, want_pairs=False):
    """(c [n_rays, 3] f32, [nodes entered, planes intersected, of those visible], pairs).  pairs: [(ray indices, plane id, visible mask, contributions)]."""
    n = d.shape[0]
    c = np.zeros((n, 3), np.float32)
    counts = [0, 0, 0]
    pairs = []

    def visit(node_id, rays):
        node = tree["nodes"][node_id]
        rays = rays[_box_entered(node["lo"], node["hi"], o[rays], d[rays], tfar[rays])]
        counts[0] += rays.shape[0]
        if rays.shape[0] == 0:
            return
        if node["left"] is None and node["right"] is None:
            for place in range(node["first"], node["first"] + node["count"]):
                p = int(tree["order"][place])
                ok, vis, val = g.hits(p, o[rays], d[rays], tfar[rays])
                hit = rays[ok]
                if hit.shape[0] == 0:
                    continue
                counts[1] += hit.shape[0]
                counts[2] += int(vis.sum())
                c[hit[vis]] = c[hit[vis]] + val
                if want_pairs:
                    pairs.append((hit, p, vis, val))
            return
        if node["right"] is not None:           # pushed last, popped first
            visit(node["right"], rays)
        if node["left"] is not None:
            visit(node["left"], rays)

    if tree["root"] is not None:
        visit(tree["root"], np.arange(n))
    return c, counts, pairs


def brute_pairs(g, o, d, tfar):
    """Every plane against every ray, no tree: [(ray indices, plane id, visible mask, contributions)] in plane order."""
    out = []
    rays = np.arange(d.shape[0])
    for p in range(len(g.planes)):
        ok, vis, val = g.hits(p, o, d, tfar)
        if ok.any():
            out.append((rays[ok], p, vis, val))
    return out


# ---- the camera loop (436-611)
def render(sc, sd, words, n_gen, strategy, seeds, spp=1, seed_variant=0, shard_index=0, shard_count=1, want_pairs=False):
    """(image HxWx3 f32, the counters rl_render_plane_single reports, detail)."""
    planes = [plane_from_words(w) for w in np.asarray(words, np.uint32).reshape(-1, api.PLANE_WORDS)]
    g = Gatherer(sc, sd, planes, n_gen, strategy)
    tree = build_tree(planes)
    px, py, o, d, tfar = camera_samples(sc, sd, seeds, spp, seed_variant, shard_index, shard_count)
    c, counts, pairs = gather(tree, g, o, d, tfar, want_pairs)
    img = np.zeros((sd.height, sd.width, 3), np.float32)
    n = d.shape[0]
    acc = np.zeros((n // spp, 3), np.float32)
    for s in range(spp):                                   # im_block.accumulate in sample order
        acc = acc + c[s::spp]
    img[py[::spp], px[::spp]] = acc * (ONE / F32(spp))     # im_block.scale(1.0 / nb_samples as f32)
    stats = {"camera_samples": n, "extension_rays": n, "rng_draws": 2 * n, "shadow_rays": counts[1], "nodes_entered": counts[0],
             "planes_intersected": counts[1], "planes_visible": counts[2]}
    return img, stats, {"tree": tree, "gatherer": g, "planes": planes, "o": o, "d": d, "tfar": tfar, "c": c, "pairs": pairs}


def compute(sd, seed=0, nb_primitive=128, strategy="average", spp=1, seed_variant=0, want_pairs=False, state=None):
    """IntegratorSinglePlane::compute seed for seed: the main sampler seeded as `-r independent:SEED` (or handed over as `state`), the plane pass, the block
    seeds from the advanced sampler, the gather."""
    sc = orc.Scene(sd)
    if state is None:
        state = list(orc.Rng(seed, seed_variant).state)
    planes, words, n_gen, after, draws, redraws = generate(sd, state, nb_primitive, strategy)
    st = after.copy()
    seeds = np.zeros(orc.lib().orc_block_count(sd.width, sd.height), np.uint64)
    orc.lib().orc_generate_block_seeds(abi.u64ptr(st), sd.width, sd.height, abi.u64ptr(seeds))
    img, stats, detail = render(sc, sd, words, n_gen, strategy, seeds, spp, seed_variant, want_pairs=want_pairs)
    return {"records": words, "n_gen": n_gen, "state": after, "draws": draws, "redraws": redraws, "seeds": seeds, "image": img, "stats": stats,
            "detail": detail, "scene": sc}


# ---- a sampler state whose second and third draws are given: the xoshiro256++ step run backwards (for the redraw test)
_M = (1 << 64) - 1


def _rotl(x, k):
    return ((x << k) | (x >> (64 - k))) & _M


def state_before(after):
    """The state one next_u64 before `after` ([4] ints)."""
    a0, a1, a2, a3 = (int(v) for v in after)
    x = a1 ^ a2                                     # = s1 ^ (s1 << 17)
    s1 = x ^ ((x << 17) & _M) ^ ((x << 34) & _M) ^ ((x << 51) & _M)
    m = a1 ^ s1                                     # = s2 ^ s0
    s3x = _rotl(a3, 64 - 45)                        # = s3 ^ s1
    s0 = a0 ^ s3x
    return [s0, s1, m ^ s0, s3x ^ s1]
