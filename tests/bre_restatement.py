"""The beam radiance estimate of IntegratorVolPrimitives restated in float32 numpy from the reference's text, the yardstick of tests/test_bre_restatement.py
and tests/test_gpu_bre_exact.py (a plain module: `from tests import bre_restatement`).

What is restated: BHVAccel::create / build and gather (src/accel.rs:458-581), AABB::intersect (src/structure.rs:849-869), Photon::aabb / intersection /
contribute (src/integrators/explicit/vol_primitives.rs:48-98), PhaseFunction::eval and HomogenousVolume::transmittance (src/volume.rs:18-28, 137-141),
Color * f32's non-finite guard, and the camera loop of IntegratorVolPrimitives::compute (vol_primitives.rs:707-790).  What is taken from the oracle's existing
entry points: the photons and the path count (Scene.vpl_generate with VPL_VOLUME), the block seeds, orc.Rng, camera_generate, trace (max_dist) and
orc_expf (orc_math_batch).

Every float operation is a float32 scalar or elementwise numpy operation in the reference's order: dot = (x x' + y y') + z z', nothing fused, powi(2) as
r * r.  The walk is vectorised over the camera samples: every sample visits the nodes in the same order (node, right subtree, left subtree: the stack pops a
node after pushing left, then right), so one pass over the tree in that order with a mask of the samples that entered each node adds every sample's photons in
the order the reference's gather returns them.  The one stated difference from the reference is the tie rule of the sort: stable (Python's sort is)."""

import numpy as np

from oracle import orc
from rustlight_amd import abi, api

F32 = np.float32
F32_MAX = np.finfo(np.float32).max
TNEAR = F32(0.0001)                 # constants::EPSILON: Ray::new's tnear


def records_of(words):
    """(pos, radiance, d_in), each [n, 3] f32, of VPL records [n, VPL_WORDS] u32."""
    w = np.ascontiguousarray(words, np.uint32).reshape(-1, api.VPL_WORDS)
    f = w.view(np.float32)
    return f[:, 4:7].copy(), f[:, 7:10].copy(), f[:, 10:13].copy()


# ---- BHVAccel::create / build (accel.rs:458-543)
def build_tree(pos, radius):
    """{"nodes": [...] in the reference's numbering (a node is pushed when its recursion returns), "root", "order"}: order[place] = the photon that stands there
    once every sort is done; a node = {"lo", "hi", "first", "count", "left", "right"}."""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    assert np.isfinite(pos).all()
    r = F32(radius)
    order = list(range(pos.shape[0]))
    nodes = []

    def build(begin, end):
        if end == begin:
            return None
        lo = np.full(3, F32_MAX, np.float32)
        hi = np.full(3, -F32_MAX, np.float32)
        for i in range(begin, end):                  # aabb = aabb.union_aabb(&self.elements[i].aabb())
            p = pos[order[i]]
            e_lo = np.minimum(np.minimum(F32_MAX, p - r), p + r)          # Photon::aabb: default().union_vec(pos - radius).union_vec(pos + radius)
            e_hi = np.maximum(np.maximum(-F32_MAX, p - r), p + r)
            lo, hi = np.minimum(lo, e_lo), np.maximum(hi, e_hi)
        if end - begin <= 4:
            nodes.append({"lo": lo, "hi": hi, "first": begin, "count": end - begin, "left": None, "right": None})
            return len(nodes) - 1
        size = hi - lo
        axis = (0 if size[0] > size[2] else 2) if size[0] > size[1] else (1 if size[1] > size[2] else 2)
        seg = order[begin:end]
        seg.sort(key=lambda i: float(pos[i, axis]))      # stable; -0.0 == +0.0
        order[begin:end] = seg
        split = (begin + end) // 2
        left = build(begin, split)
        right = build(split, end)
        nodes.append({"lo": lo, "hi": hi, "first": 0, "count": 0, "left": left, "right": right})
        return len(nodes) - 1

    root = build(0, len(order))
    return {"nodes": nodes, "root": root, "order": np.asarray(order, np.uint32)}


def visit_order(tree):
    """The node ids in the order gather's stack pops them when every box is entered."""
    out, stack = [], ([] if tree["root"] is None else [tree["root"]])
    while stack:
        n = stack.pop()
        out.append(n)
        node = tree["nodes"][n]
        if node["left"] is not None:
            stack.append(node["left"])
        if node["right"] is not None:
            stack.append(node["right"])
    return out


def sort_keys_distinct(pos):
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    return all(np.unique(pos[:, a]).shape[0] == pos.shape[0] for a in range(3))


# ---- the float32 pieces
def _expf(x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros_like(x)
    if x.size:
        orc.lib().orc_math_batch(2, x.size, abi.fptr(x.reshape(-1)), abi.fptr(x.reshape(-1)), abi.fptr(out.reshape(-1)))
    return out


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _scale(c, s):
    """Color * f32 (structure.rs: a non-finite factor gives black)."""
    s = F32(s)
    return c * s if np.isfinite(s) else np.zeros_like(c)


def _box_entered(lo, hi, o, d, tfar):
    """AABB::intersect(..).is_some() for rays (o, d, tnear = EPSILON, tfar): the loop of structure.rs:853-866, its early return kept as a mask."""
    with np.errstate(all="ignore"):
        t_min = np.full(d.shape[0], TNEAR, np.float32)
        t_max = tfar.copy()
        alive = np.ones(d.shape[0], bool)
        for a in range(3):
            inv_d = F32(1.0) / d[:, a]
            t0 = (lo[a] - o[:, a]) * inv_d
            t1 = (hi[a] - o[:, a]) * inv_d
            neg = inv_d < F32(0.0)
            t0, t1 = np.where(neg, t1, t0), np.where(neg, t0, t1)
            t_min = np.where(t0 > t_min, t0, t_min)
            t_max = np.where(t1 < t_max, t1, t_max)
            alive &= ~(t_max <= t_min)
        return alive


class _Photons:
    def __init__(self, words, n_paths, radius, medium):
        self.pos, self.rad, self.d_in = records_of(words)
        self.r = F32(radius)
        self.sigma_t = (np.asarray(medium.sigma_a, np.float32) + np.asarray(medium.sigma_s, np.float32)) * F32(1.0)
        self.hg, self.g = medium.phase != 0, F32(medium.g)
        self.weight = F32(1.0) / (F32(np.pi) * (self.r * self.r))          # 1.0 / (PI * self.radius.powi(2))
        self.norm = F32(1.0) / F32(n_paths)                                 # 1.0 / nb_path_shot as f32

    def test(self, p, o, d, tfar):
        """Photon::intersection for photon p on rays (o, d, tfar): (accepted mask, dot)."""
        pos = self.pos[p]
        dot = _dot(pos[0] - o[:, 0], pos[1] - o[:, 1], pos[2] - o[:, 2], d[:, 0], d[:, 1], d[:, 2])
        px, py, pz = o[:, 0] + d[:, 0] * dot, o[:, 1] + d[:, 1] * dot, o[:, 2] + d[:, 2] * dot
        ex, ey, ez = pos[0] - px, pos[1] - py, pos[2] - pz
        dist = _dot(ex, ey, ez, ex, ey, ez)
        return ~((dot <= F32(0.0)) | (dot > tfar)) & ~(dist > self.r * self.r), dot

    def contribute(self, p, d, dot):
        """Photon::contribute(ray, m, dist) * norm_photon, [k, 3]."""
        tau = np.where(np.isfinite(dot)[:, None], self.sigma_t[None, :] * dot[:, None], F32(0.0)).astype(np.float32)     # sigma_t * r.tfar
        trans = _expf(-tau)
        if self.hg:
            din = self.d_in[p]
            cos = _dot(-d[:, 0], -d[:, 1], -d[:, 2], din[0], din[1], din[2])
            g = self.g
            tmp = F32(1.0) + g * g + F32(2.0) * g * cos
            phase = F32(1.0 / np.pi) * F32(0.25) * (F32(1.0) - g * g) / (tmp * np.sqrt(tmp))
        else:
            phase = np.full(d.shape[0], F32(1.0) / (F32(np.pi) * F32(4.0)), np.float32)
        c = (self.rad[p][None, :] * trans) * phase[:, None]
        return _scale(_scale(c, self.weight), self.norm)


# ---- BHVAccel::gather (accel.rs:545-581) and the sum of vol_primitives.rs:765-771, over all rays at once
def gather(tree, photons, o, d, tfar, want_pairs=False):
    """(c [n_rays, 3] f32, nodes entered, photons gathered, pairs).  pairs (want_pairs): [(ray indices, photon id, contributions [k, 3])] in gather order."""
    n = d.shape[0]
    c = np.zeros((n, 3), np.float32)
    counts = [0, 0]
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
                ok, dot = photons.test(p, o[rays], d[rays], tfar[rays])
                hit = rays[ok]
                if hit.shape[0] == 0:
                    continue
                counts[1] += hit.shape[0]
                val = photons.contribute(p, d[hit], dot[ok])
                c[hit] = c[hit] + val
                if want_pairs:
                    pairs.append((hit, p, val))
            return
        if node["right"] is not None:           # pushed last, popped first
            visit(node["right"], rays)
        if node["left"] is not None:
            visit(node["left"], rays)

    if tree["root"] is not None:
        visit(tree["root"], np.arange(n))
    return c, counts[0], counts[1], pairs


def brute_pairs(photons, o, d, tfar):
    """Every photon against every ray, no tree: [(ray indices, photon id, contributions)] in photon order."""
    out = []
    rays = np.arange(d.shape[0])
    for p in range(photons.pos.shape[0]):
        ok, dot = photons.test(p, o, d, tfar)
        if ok.any():
            out.append((rays[ok], p, photons.contribute(p, d[ok], dot[ok])))
    return out


# ---- the camera loop (vol_primitives.rs:711-790)
def camera_samples(sc, sd, seeds, spp, seed_variant=0, shard_index=0, shard_count=1):
    """The rays of every camera sample of the shard's blocks, in the order the reference takes them: (pixel x, pixel y, o, d, tfar)."""
    nby = (sd.height + 15) // 16
    px, py, os_, ds = [], [], [], []
    for b, seed in enumerate(np.asarray(seeds, np.uint64)):
        if b % shard_count != shard_index:
            continue
        bx, by = (b // nby) * 16, (b % nby) * 16
        bw, bh = min(16, sd.width - bx), min(16, sd.height - by)
        rng = orc.Rng(int(seed), seed_variant)
        for ix in range(bw):
            for iy in range(bh):
                for _ in range(spp):
                    u = F32(bx + ix) + F32(rng.next_f32())
                    v = F32(by + iy) + F32(rng.next_f32())
                    o, d = sc.camera_generate(float(u), float(v))
                    px.append(bx + ix); py.append(by + iy); os_.append(o); ds.append(d)
    o, d = np.asarray(os_, np.float32).reshape(-1, 3), np.asarray(ds, np.float32).reshape(-1, 3)
    t, _, _, mesh, _ = sc.trace(o, d)
    tfar = np.where(mesh >= 0, t, F32_MAX).astype(np.float32)         # the closest hit's dist, f32::MAX on a miss
    return np.asarray(px), np.asarray(py), o, d, tfar


def render(sc, sd, words, n_paths, seeds, spp=1, radius=api.PHOTON_RADIUS_DEFAULT, seed_variant=0, shard_index=0, shard_count=1, want_pairs=False):
    """(image HxWx3 f32, {camera_samples, extension_rays, rng_draws, nodes_entered, photons_gathered}, detail) as rl_render_bre reports them.
    detail: tree, photons, rays and per-sample sums, for the tests that look inside."""
    photons = _Photons(words, n_paths, radius, sd.medium)
    tree = build_tree(photons.pos, radius)
    px, py, o, d, tfar = camera_samples(sc, sd, seeds, spp, seed_variant, shard_index, shard_count)
    c, entered, gathered, pairs = gather(tree, photons, o, d, tfar, want_pairs)
    img = np.zeros((sd.height, sd.width, 3), np.float32)
    n = d.shape[0]
    acc = np.zeros((n // spp, 3), np.float32)
    for s in range(spp):                                   # im_block.accumulate in sample order
        acc = acc + c[s::spp]
    img[py[::spp], px[::spp]] = acc * (F32(1.0) / F32(spp))     # im_block.scale(1.0 / nb_samples as f32)
    stats = {"camera_samples": n, "extension_rays": n, "rng_draws": 2 * n, "nodes_entered": entered, "photons_gathered": gathered}
    return img, stats, {"tree": tree, "photons": photons, "o": o, "d": d, "tfar": tfar, "c": c, "pairs": pairs}


def compute(sd, seed=0, nb_primitive=128, spp=1, max_depth=None, rr_depth=0, radius=api.PHOTON_RADIUS_DEFAULT, seed_variant=0, want_pairs=False):
    """IntegratorVolPrimitives::compute (BRE) seed for seed: the main sampler seeded as `-r independent:SEED`, the photon pass, the block seeds from the
    advanced sampler, the gather."""
    sc = orc.Scene(sd)
    rng = orc.Rng(seed, seed_variant)
    rec, n_paths, after, gstats = sc.vpl_generate(rng.state, nb_primitive, max_depth, rr_depth, api.VPL_VOLUME)
    st = after.copy()
    seeds = np.zeros(orc.lib().orc_block_count(sd.width, sd.height), np.uint64)
    orc.lib().orc_generate_block_seeds(abi.u64ptr(st), sd.width, sd.height, abi.u64ptr(seeds))
    img, stats, detail = render(sc, sd, rec, n_paths, seeds, spp, radius, seed_variant, want_pairs=want_pairs)
    return {"records": rec, "n_paths": n_paths, "state": after, "gen_stats": gstats, "seeds": seeds, "image": img, "stats": stats, "detail": detail, "scene": sc}
