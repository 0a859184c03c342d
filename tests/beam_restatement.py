"""The photon beams of IntegratorVolPrimitives restated in float32 numpy from the reference's text, the yardstick of tests/test_beam_restatement.py and the
tests/test_gpu_beam_*.py files (a plain module: `from tests import beam_restatement`).

What is restated: the split into sub-beams (src/integrators/explicit/vol_primitives.rs:647-684), PhotonBeam::aabb / position / intersection / contribute
(:123-199), BHVAccel::create / build and gather (src/accel.rs:458-581) and the `Beams` arm of the camera loop (vol_primitives.rs:705-790).  What is shared
with tests/bre_restatement.py, which restates them for the photons: AABB::intersect, Color * f32's non-finite guard, orc_expf, the camera samples (block
seeds, orc.Rng, camera_generate, the oracle's trace for max_dist) and the visiting order.  The beams themselves are records of RL_BEAM_WORDS u32 (o, length,
d, flags, radiance, path): tests/test_gpu_beam_records.py holds the device's to the oracle's light paths.

Every float operation is a float32 scalar or elementwise numpy operation in the reference's order: dot = (x x' + y y') + z z', nothing fused.  The walk is
vectorised over the camera samples as in bre_restatement.  The one stated difference from the reference is the tie rule of the sort: stable."""

import numpy as np

from rustlight_amd import api
from tests import bre_restatement as B

F32 = np.float32
F32_MAX = B.F32_MAX
TNEAR = B.TNEAR
SPLIT = 5


def beam_words(o, length, d, radiance, from_surface=True, path=0):
    """Records [n, BEAM_WORDS] u32 of hand-made beams."""
    o = np.asarray(o, np.float32).reshape(-1, 3)
    n = o.shape[0]
    w = np.zeros((n, api.BEAM_WORDS), np.uint32)
    f = w.view(np.float32)
    f[:, 0:3] = o
    f[:, 3] = np.broadcast_to(np.asarray(length, np.float32), (n,))
    f[:, 4:7] = np.broadcast_to(np.asarray(d, np.float32).reshape(-1, 3), (n, 3))
    w[:, 7] = np.broadcast_to(np.asarray(from_surface, bool), (n,)).astype(np.uint32)
    f[:, 8:11] = np.broadcast_to(np.asarray(radiance, np.float32).reshape(-1, 3), (n, 3))
    w[:, 11] = np.broadcast_to(np.asarray(path, np.uint32), (n,))
    return w


def records_of(words):
    """(o [n, 3], length [n], d [n, 3], radiance [n, 3]) f32 of beam records."""
    f = np.ascontiguousarray(words, np.uint32).reshape(-1, api.BEAM_WORDS).view(np.float32)
    return f[:, 0:3].copy(), f[:, 3].copy(), f[:, 4:7].copy(), f[:, 8:11].copy()


# ---- the split (vol_primitives.rs:647-684)
def split(words):
    """The sub-beams [n_sub, BEAM_WORDS] u32 in beam order: records of the same layout with o and length replaced."""
    words = np.ascontiguousarray(words, np.uint32).reshape(-1, api.BEAM_WORDS)
    o, length, d, _ = records_of(words)
    n = words.shape[0]
    assert np.isfinite(o).all() and np.isfinite(d).all() and np.isfinite(length).all()
    total = F32(0.0)
    for v in length:                                          # beams.iter().map(|b| b.length).sum::<f32>()
        total = F32(total + v)
    avg_split = total / F32(n * SPLIT)                        # / (beams.len() * SPLIT) as f32
    assert np.isfinite(avg_split) and avg_split != 0
    out = []
    for i in range(n):
        number_split = min(max(int(np.ceil(length[i] / avg_split)), 0), 0xffffffff)      # (b.length / avg_split).ceil() as u32
        if number_split == 0:
            continue
        new_length = length[i] / F32(number_split)
        for s in range(number_split):
            rec = words[i].copy()
            rec.view(np.float32)[0:3] = o[i] + d[i] * F32(s) * new_length           # b.o + b.d * (i as f32) * new_length
            rec.view(np.float32)[3] = new_length
            out.append(rec)
    return np.asarray(out, np.uint32).reshape(-1, api.BEAM_WORDS)


# ---- PhotonBeam::aabb / position (vol_primitives.rs:123-136) and BHVAccel::create / build (accel.rs:458-543)
def element_boxes(sub, radius):
    """(lo [n, 3], hi [n, 3], key [n, 3]) f32 of sub-beam records."""
    o, length, d, _ = records_of(sub)
    r = F32(radius)
    end = o + d * length[:, None]                             # self.o + self.d * self.length
    corners = [o - r, o + r, end - r, end + r]
    lo, hi = np.full_like(o, F32_MAX), np.full_like(o, -F32_MAX)
    for c in corners:                                         # aabb.union_vec, four times
        lo, hi = np.minimum(lo, c), np.maximum(hi, c)
    key = o + d * length[:, None] * F32(0.5)                  # self.o + self.d * self.length * 0.5
    return lo.astype(np.float32), hi.astype(np.float32), key.astype(np.float32)


def build_tree(sub, radius):
    """bre_restatement.build_tree's dictionary over the sub-beams' boxes and keys."""
    e_lo, e_hi, key = element_boxes(sub, radius)
    assert np.isfinite(e_lo).all() and np.isfinite(e_hi).all() and np.isfinite(key).all()
    order = list(range(e_lo.shape[0]))
    nodes = []

    def build(begin, end):
        if end == begin:
            return None
        lo = np.full(3, F32_MAX, np.float32)
        hi = np.full(3, -F32_MAX, np.float32)
        for i in range(begin, end):                           # aabb = aabb.union_aabb(&self.elements[i].aabb())
            lo, hi = np.minimum(lo, e_lo[order[i]]), np.maximum(hi, e_hi[order[i]])
        if end - begin <= 4:
            nodes.append({"lo": lo, "hi": hi, "first": begin, "count": end - begin, "left": None, "right": None})
            return len(nodes) - 1
        size = hi - lo
        axis = (0 if size[0] > size[2] else 2) if size[0] > size[1] else (1 if size[1] > size[2] else 2)
        seg = order[begin:end]
        seg.sort(key=lambda i: float(key[i, axis]))          # stable; -0.0 == +0.0
        order[begin:end] = seg
        split_at = (begin + end) // 2
        left = build(begin, split_at)
        right = build(split_at, end)
        nodes.append({"lo": lo, "hi": hi, "first": 0, "count": 0, "left": left, "right": right})
        return len(nodes) - 1

    root = build(0, len(order))
    return {"nodes": nodes, "root": root, "order": np.asarray(order, np.uint32)}


def tree_arrays(tree):
    """(boxes [n, 6] f32, links [n, 3] u32 = skip, first, count, order) as rl_beam_tree_build writes them: nodes in visiting order."""
    visit = B.visit_order(tree)
    size = {}
    for n in reversed(visit):
        node = tree["nodes"][n]
        size[n] = 1 + sum(size[k] for k in (node["left"], node["right"]) if k is not None)
    boxes, links = np.zeros((len(visit), 6), np.float32), np.zeros((len(visit), 3), np.uint32)
    for i, n in enumerate(visit):
        node = tree["nodes"][n]
        boxes[i] = np.concatenate([node["lo"], node["hi"]])
        links[i] = (i + size[n], node["first"], node["count"])
    return boxes, links, tree["order"]


def sort_keys_distinct(sub, radius=0.1):
    key = element_boxes(sub, radius)[2]
    return all(np.unique(key[:, a]).shape[0] == key.shape[0] for a in range(3))


# ---- PhotonBeam::intersection / contribute (vol_primitives.rs:140-199)
class Beams:
    def __init__(self, sub, n_paths, radius, medium):
        self.o, self.length, self.d, self.rad = records_of(sub)
        self.r = F32(radius)
        self.sigma_t = (np.asarray(medium.sigma_a, np.float32) + np.asarray(medium.sigma_s, np.float32)) * F32(1.0)
        self.sigma_s = np.asarray(medium.sigma_s, np.float32)
        self.norm = F32(1.0) / F32(n_paths)                                 # 1.0 / nb_path_shot as f32

    def test(self, b, o, d, tfar):
        """PhotonBeam::intersection for sub-beam b on rays (o, d, tfar): (accepted mask, u, v, w, sin_theta)."""
        bo, bd = self.o[b], self.d[b]
        with np.errstate(all="ignore"):
            cx = d[:, 1] * bd[2] - d[:, 2] * bd[1]                          # r.d.cross(self.d)
            cy = d[:, 2] * bd[0] - d[:, 0] * bd[2]
            cz = d[:, 0] * bd[1] - d[:, 1] * bd[0]
            sin_theta_sqr = B._dot(cx, cy, cz, cx, cy, cz)
            ad = B._dot(bo[0] - o[:, 0], bo[1] - o[:, 1], bo[2] - o[:, 2], cx, cy, cz)
            ok = ~(ad * ad >= (self.r * self.r) * sin_theta_sqr)
            d1d2 = B._dot(d[:, 0], d[:, 1], d[:, 2], bd[0], bd[1], bd[2])
            m1 = d1d2 * d1d2 - F32(1.0)
            ok &= ~((m1 < F32(1e-5)) & (m1 > F32(-1e-5)))
            d1o1 = B._dot(d[:, 0], d[:, 1], d[:, 2], o[:, 0], o[:, 1], o[:, 2])
            d1o2 = B._dot(d[:, 0], d[:, 1], d[:, 2], bo[0], bo[1], bo[2])
            d2o1 = B._dot(bd[0], bd[1], bd[2], o[:, 0], o[:, 1], o[:, 2])
            d2o2 = B._dot(bd[0], bd[1], bd[2], bo[0], bo[1], bo[2])
            w = (d1o1 - d1o2 - d1d2 * (d2o1 - d2o2)) / m1
            ok &= ~((w <= TNEAR) | (w >= tfar))
            v = (w + d1o1 - d1o2) / d1d2
            ok &= ~((v <= F32(0.0)) | (v >= self.length[b]) | ~np.isfinite(v))
            sin_theta = np.sqrt(sin_theta_sqr)
            u = np.abs(ad) / sin_theta
        return ok, u.astype(np.float32), v.astype(np.float32), w.astype(np.float32), sin_theta.astype(np.float32)

    def contribute(self, b, w, sin_theta):
        """PhotonBeam::contribute(ray, m, its) * norm_photon, [k, 3]."""
        tau = np.where(np.isfinite(w)[:, None], self.sigma_t[None, :] * w[:, None], F32(0.0)).astype(np.float32)     # sigma_t * ray_tr.tfar
        trans = B._expf(-tau)
        phase_func = self.sigma_s * (F32(1.0) / (F32(np.pi) * F32(4.0)))    # m.sigma_s * Isotropic.eval(..)
        with np.errstate(all="ignore"):
            weight = (F32(1.0) / sin_theta) * (F32(0.5) / self.r)
            c = (self.rad[b][None, :] * trans) * phase_func[None, :]
            c = np.where(np.isfinite(weight)[:, None], c * weight[:, None], F32(0.0)).astype(np.float32)       # Color * f32
        return B._scale(c, self.norm)


# ---- BHVAccel::gather (accel.rs:545-581) and the sum of vol_primitives.rs:734-740, over all rays at once
def gather(tree, beams, o, d, tfar, want_pairs=False):
    """(c [n_rays, 3] f32, nodes entered, beams accepted, pairs).  pairs (want_pairs): [(ray indices, sub-beam id, contributions [k, 3])] in gather order."""
    n = d.shape[0]
    c = np.zeros((n, 3), np.float32)
    counts = [0, 0]
    pairs = []

    def visit(node_id, rays):
        node = tree["nodes"][node_id]
        rays = rays[B._box_entered(node["lo"], node["hi"], o[rays], d[rays], tfar[rays])]
        counts[0] += rays.shape[0]
        if rays.shape[0] == 0:
            return
        if node["left"] is None and node["right"] is None:
            for place in range(node["first"], node["first"] + node["count"]):
                b = int(tree["order"][place])
                ok, _, _, w, sin_theta = beams.test(b, o[rays], d[rays], tfar[rays])
                hit = rays[ok]
                if hit.shape[0] == 0:
                    continue
                counts[1] += hit.shape[0]
                val = beams.contribute(b, w[ok], sin_theta[ok])
                c[hit] = c[hit] + val
                if want_pairs:
                    pairs.append((hit, b, val))
            return
        if node["right"] is not None:           # pushed last, popped first
            visit(node["right"], rays)
        if node["left"] is not None:
            visit(node["left"], rays)

    if tree["root"] is not None:
        visit(tree["root"], np.arange(n))
    return c, counts[0], counts[1], pairs


KEYS = ("camera_samples", "extension_rays", "rng_draws", "nodes_entered", "beams_accepted")


def render_rays(sd, words, n_paths, radius, px, py, o, d, tfar, spp, want_pairs=False):
    """The camera loop over given camera samples (spp consecutive ones per pixel)."""
    sub = split(words)
    beams = Beams(sub, n_paths, radius, sd.medium)
    tree = build_tree(sub, radius)
    c, entered, accepted, pairs = gather(tree, beams, o, d, tfar, want_pairs)
    img = np.zeros((sd.height, sd.width, 3), np.float32)
    n = d.shape[0]
    acc = np.zeros((n // spp, 3), np.float32)
    for s in range(spp):                                   # im_block.accumulate in sample order
        acc = acc + c[s::spp]
    img[py[::spp], px[::spp]] = acc * (F32(1.0) / F32(spp))     # im_block.scale(1.0 / nb_samples as f32)
    stats = {"camera_samples": n, "extension_rays": n, "rng_draws": 2 * n, "nodes_entered": entered, "beams_accepted": accepted}
    return img, stats, {"sub": sub, "tree": tree, "beams": beams, "o": o, "d": d, "tfar": tfar, "c": c, "pairs": pairs}


def render(sc, sd, words, n_paths, seeds, spp=1, radius=api.PHOTON_RADIUS_DEFAULT, seed_variant=0, shard_index=0, shard_count=1, want_pairs=False):
    """(image HxWx3 f32, the counters of KEYS, detail) as rl_render_beams reports them, from beam records `words` of n_paths light paths."""
    px, py, o, d, tfar = B.camera_samples(sc, sd, seeds, spp, seed_variant, shard_index, shard_count)
    return render_rays(sd, words, n_paths, radius, px, py, o, d, tfar, spp, want_pairs)
