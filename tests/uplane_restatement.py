"""IntegratorSinglePlaneUncorrelated restated in float32 numpy from the reference's text (src/integrators/explicit/uncorrelated_plane_single.rs), the yardstick
of tests/test_uplane_restatement.py, tests/test_gpu_uplane_exact.py and tests/test_gpu_uplane_quadrature.py (a plain module: `from tests import
uplane_restatement`).

The loop (:86-316): per block, ix, iy, sample; per camera sample 2 draws for the jitter, camera.generate and accel.trace (tfar = the hit's distance or f32::MAX),
then per plane j < nb_primitive one draw for id_emitter (clamped to the last light, plane-single's stated deviation), one more under average / discrete_mis
for the plane type (< 1/3 UV, < 2/3 VT, else UT: ONE plane of a random type), cosine_sample_hemisphere(next2d()) again while z == 0, one draw for the distance,
two for `sample`, one for alpha; SinglePhotonPlane::new, intersection, light_position, accel.visible, the transmittance, rho = Isotropic, the strategy's w and
flux, c += w * rho * transmittance * sigma_s * flux * n_lights * (1 / nb_primitive); the samples of a pixel are added in order and scaled by 1 / spp.

Two forms.  walk_block is the literal scalar walk: one orc.Rng, and plane_single_restatement's own rect_lights, cosine_sample_hemisphere, frame_to_world,
plane_new, intersect, light_position, contrib, discrete_mis_weights, w_cmis and sigma_t_of, plane after plane.  render is the same arithmetic with every
(sample, plane) pair of a block as one array element: the block's stream comes from a numpy xoshiro256++ (stream(), checked against orc.Rng by
tests/test_uplane_restatement.py, which also holds the two forms equal), a pair's draws sit at fixed places in it, and a direction that is drawn again moves
every later place by 2 (resolved pair by pair, first redraw first).  Every float operation is a float32 elementwise operation in the reference's order, as in
plane_single_restatement.  camera_generate, trace, visible and orc_math_batch (sin, cos, exp, log) are the oracle's."""

import numpy as np

from oracle import orc
from tests import plane_single_restatement as R
from tests.bre_restatement import F32, F32_MAX, _expf

PI, FRAC_PI_2, FRAC_PI_4, ONE, ZERO = R.PI, R.FRAC_PI_2, R.FRAC_PI_4, R.ONE, R.ZERO
UV, VT, UT, UALPHAT = R.UV, R.VT, R.UT, R.UALPHAT
STRATEGIES = R.STRATEGIES
SINGLE_TYPE = {"uv": UV, "vt": VT, "ut": UT, "ualpha": UALPHAT, "cmis": UALPHAT}
# The plane counts of the image fixtures (cbox_medium(32, 24, 1.0), seed 3, spp 2): the smallest of 64, 256, 512 at which the image is non-zero in a quarter of
# its pixels (uv at 256 and vt at 64 are not) — tests/test_uplane_restatement.py asserts the quarter of every one
FIXTURE_NB = {"uv": 512, "vt": 256, "ut": 64, "average": 64, "discrete_mis": 64, "ualpha": 64, "cmis": 64}
# The redraw cases: (block seed, strategy, nb_primitive, spp, lane, sample, plane).  Rng(303, 0) draws exactly 0.0 at index 91307 and Rng(196, 0) at index 226623
REDRAW_CASES = [(303, "ut", 80, 2, 81, 0, 37), (303, "average", 33, 2, 171, 1, 8), (196, "ut", 32, 4, 250, 2, 24), (196, "discrete_mis", 121, 1, 233, 0, 76)]


def picks_type(strategy):
    return strategy in ("average", "discrete_mis")


def draws_per_plane(strategy):
    return 8 if picks_type(strategy) else 7


def draws_per_sample(nb_primitive, strategy):
    return 2 + nb_primitive * draws_per_plane(strategy)


# ---- xoshiro256++ (SmallRng of rand 0.8.5) in numpy: many substreams of one stream stepped side by side
_U = np.uint64
_SUB = 2048                      # draws per substream


def _rotl(x, k):
    return (x << _U(k)) | (x >> _U(64 - k))


def _step(s):
    """One next_u64 of every column of s [4, n] u64: (outputs, next states)."""
    s0, s1, s2, s3 = s
    out = _rotl(s0 + s3, 23) + s0
    t = s1 << _U(17)
    s2 = s2 ^ s0
    s3 = s3 ^ s1
    s1 = s1 ^ s2
    s0 = s0 ^ s3
    s2 = s2 ^ t
    s3 = _rotl(s3, 45)
    return out, np.stack([s0, s1, s2, s3])


def _bits(s):
    """s [4, n] u64 -> [256, n] f32 of 0 / 1, bit 64 w + b of a state in row 64 w + b."""
    n = s.shape[1]
    b = np.unpackbits(np.ascontiguousarray(s.T).view(np.uint8).reshape(n, 32), axis=1, bitorder="little")
    return b.T.astype(np.float32)


def _unbits(b):
    n = b.shape[1]
    return np.ascontiguousarray(np.packbits(b.T.astype(np.uint8), axis=1, bitorder="little")).view(np.uint64).reshape(n, 4).T.copy()


_JUMP = {}


def _jump_matrix(steps):
    """The state transition over `steps` draws as a 256 x 256 matrix over GF(2) (the update is linear: xor, shift, rotate)."""
    if steps not in _JUMP:
        basis = np.zeros((4, 256), np.uint64)
        for i in range(256):
            basis[i // 64, i] = _U(1) << _U(i % 64)
        t = _bits(_step(basis)[1])
        acc, k = np.eye(256, dtype=np.float32), steps
        while k:
            if k & 1:
                acc = np.mod(t @ acc, 2.0)
            t = np.mod(t @ t, 2.0)
            k >>= 1
        _JUMP[steps] = acc
    return _JUMP[steps]


def _state_bits(seed, variant):
    return _bits(np.array(list(orc.Rng(int(seed), variant).state), np.uint64).reshape(4, 1))


def _outputs(seed, variant, n, width=16384):
    """The first n next_u64 of orc.Rng(seed, variant) in pieces: yields (c0, buf [_SUB, m] u64), buf[i, c] = draw (c0 + c) * _SUB + i."""
    n_sub = max(1, -(-n // _SUB))
    starts, jump = _state_bits(seed, variant), _jump_matrix(_SUB)          # the substreams' first states: 1, 2, 4, ... of them
    while starts.shape[1] < n_sub:
        starts = np.concatenate([starts, np.mod(jump @ starts, 2.0)], axis=1)
        jump = np.mod(jump @ jump, 2.0)
    for c0 in range(0, n_sub, width):
        s0, s1, s2, s3 = (np.ascontiguousarray(r) for r in _unbits(starts[:, c0:min(c0 + width, n_sub)]))
        buf = np.empty((_SUB, s0.shape[0]), np.uint64)
        t = np.empty_like(s0)
        with np.errstate(over="ignore"):
            for i in range(_SUB):
                np.add(s0, s3, out=t)
                buf[i] = _rotl(t, 23)
                buf[i] += s0
                np.left_shift(s1, _U(17), out=t)
                s2 ^= s0
                s3 ^= s1
                s1 ^= s2
                s0 ^= s3
                s2 ^= t
                s3 = _rotl(s3, 45)
        yield c0, buf


def stream(seed, variant, n):
    """The first n next_f32 of orc.Rng(seed, variant), [n] f32."""
    out = np.empty(max(1, -(-n // _SUB)) * _SUB, np.float32)
    for c0, buf in _outputs(seed, variant, n):
        u = buf.T.reshape(-1)
        out[c0 * _SUB:c0 * _SUB + u.shape[0]] = (u >> _U(40)).astype(np.float32) * F32(1.0 / 16777216.0)      # (next_u64() >> 32) >> 8, * 2^-24
    return out[:n]


def zero_draws(seed, variant, n):
    """The indices below n at which orc.Rng(seed, variant) draws exactly 0.0, without keeping the stream."""
    found = [np.zeros(0, np.int64)]
    for c0, buf in _outputs(seed, variant, n):
        i, c = np.nonzero(buf < (_U(1) << _U(40)))                  # next_f32 is (next_u64() >> 40) * 2^-24
        found.append((c0 + c.astype(np.int64)) * _SUB + i)
    z = np.sort(np.concatenate(found))
    return z[z < n]


def draws_at(seed, variant, i, count):
    """next_f32 number i .. i + count - 1 of orc.Rng(seed, variant): the stream entered by a jump."""
    st = _unbits(np.mod(_jump_matrix(int(i)) @ _state_bits(seed, variant), 2.0))
    r = orc.Rng.from_state([int(v) for v in st[:, 0]])
    return np.asarray([r.next_f32() for _ in range(count)], np.float32)


# ---- the float32 pieces over arrays of pairs
def _hemisphere(ux, uy):
    """cosine_sample_hemisphere / concentric_sample_disk (src/math.rs:37-65, 357-375) elementwise: [n, 3]."""
    with np.errstate(all="ignore"):
        ox, oy = ux * F32(2.0) - ONE, uy * F32(2.0) - ONE
        first = np.abs(ox) > np.abs(oy)
        r = np.where(first, ox, oy)
        theta = np.where(first, FRAC_PI_4 * (oy / ox), FRAC_PI_2 - FRAC_PI_4 * (ox / oy)).astype(np.float32)
        dx, dy = R._cos(theta) * r, R._sin(theta) * r
        zero = (ox == ZERO) & (oy == ZERO)
        dx, dy = np.where(zero, ZERO, dx).astype(np.float32), np.where(zero, ZERO, dy).astype(np.float32)
        z = np.sqrt(np.fmax(ZERO, ONE - dx * dx - dy * dy)).astype(np.float32)
    return np.stack([dx, dy, z], axis=-1)


class _Lights:
    """The rectangular lights as arrays indexed by id_emitter, with Frame::new(normal)'s two tangents (src/math.rs: the lines of R.frame_to_world)."""

    def __init__(self, lights):
        self.n = len(lights)
        for k in ("o", "u", "v", "emission"):
            setattr(self, k, np.asarray([getattr(l, k) for l in lights], np.float32).reshape(-1, 3))
        self.normal = np.asarray([l.n for l in lights], np.float32).reshape(-1, 3)
        self.u_l = np.asarray([l.u_l for l in lights], np.float32)
        self.v_l = np.asarray([l.v_l for l in lights], np.float32)
        self.fx, self.fy = np.zeros((self.n, 3), np.float32), np.zeros((self.n, 3), np.float32)
        for i, l in enumerate(lights):
            n = l.n
            sign = F32(np.copysign(1.0, n[2]))
            a = F32(-1.0) / (sign + n[2])
            b = n[0] * n[1] * a
            self.fx[i] = R._v([ONE + sign * n[0] * n[0] * a, sign * b, -sign * n[0]])
            self.fy[i] = R._v([b, sign + n[1] * n[1] * a, -n[1]])


def _col(a):
    return a[:, None]


def _make_planes(L, ids, types, d, sample, alpha, t_sampled, sigma_s):
    """SinglePhotonPlane::new (plane_single.rs:177-277) for every pair: dict of o, d0, d1 [n, 3], l0, l1 [n], weight [n, 3]."""
    n = ids.shape[0]
    out = {k: np.zeros((n, 3), np.float32) for k in ("o", "d0", "d1", "weight")}
    out["l0"], out["l1"] = np.zeros(n, np.float32), np.zeros(n, np.float32)
    lo, lu, lv, em, ul, vl = L.o[ids], L.u[ids], L.v[ids], L.emission[ids], L.u_l[ids], L.v_l[ids]
    sx, sy = sample[:, 0], sample[:, 1]
    with np.errstate(all="ignore"):
        m = types == UV
        if m.any():
            out["o"][m] = lo[m] + d[m] * _col(t_sampled[m])
            out["d0"][m], out["d1"][m], out["l0"][m], out["l1"][m] = lu[m], lv[m], ul[m], vl[m]
            out["weight"][m] = (PI * em[m]) / sigma_s[None, :]
        m = types == VT
        if m.any():
            out["o"][m] = lo[m] + lu[m] * _col(ul[m]) * _col(sx[m])
            out["d0"][m], out["d1"][m], out["l0"][m], out["l1"][m] = lv[m], d[m], vl[m], t_sampled[m]
            out["weight"][m] = _col(PI * ul[m]) * em[m]
        m = types == UT
        if m.any():
            out["o"][m] = lo[m] + lv[m] * _col(vl[m]) * _col(sy[m])
            out["d0"][m], out["d1"][m], out["l0"][m], out["l1"][m] = lu[m], d[m], ul[m], t_sampled[m]
            out["weight"][m] = _col(PI * vl[m]) * em[m]
        m = types == UALPHAT
        if m.any():
            a = PI * alpha[m]
            o2x, o2y = sx[m] * ul[m], sy[m] * vl[m]
            dx, dy = R._cos(a), R._sin(a)

            def plane2d_its(ddx, ddy):
                t0x, t0y = (-o2x) / ddx, (-o2y) / ddy
                t1x, t1y = (ul[m] - o2x) / ddx, (vl[m] - o2y) / ddy
                t = np.fmin(np.fmax(t0x, t1x), np.fmax(t0y, t1y))
                return o2x + ddx * t, o2y + ddy * t

            p1x, p1y = plane2d_its(dx, dy)
            p2x, p2y = plane2d_its(-dx, -dy)
            p1 = lo[m] + _col(p1x) * lu[m] + _col(p1y) * lv[m]
            p2 = lo[m] + _col(p2x) * lu[m] + _col(p2y) * lv[m]
            u_plane = (p2 - p1).astype(np.float32)
            length = R._mag(u_plane)
            out["o"][m], out["d0"][m], out["d1"][m], out["l0"][m], out["l1"][m] = p1, u_plane / _col(length), d[m], length, t_sampled[m]
            out["weight"][m] = R._div_guarded((PI * em[m]) * _col(ul[m] * vl[m]), length)
    return out


def _intersect(pl, o, d, tfar):
    """BVHElement::intersection (plane_single.rs:121-160) of pair k's plane with pair k's ray: (accepted, t_cam, t0, t1) — R.intersect, one plane per ray."""
    with np.errstate(all="ignore"):
        e0, e1 = pl["d0"] * _col(pl["l0"]), pl["d1"] * _col(pl["l1"])
        p = R._cross(d, e1)
        det = R._dot(e0, p)
        ok = ~(np.abs(det) < F32(1e-5))
        inv_det = ONE / det
        t = (o - pl["o"]).astype(np.float32)
        t0 = R._dot(t, p) * inv_det
        ok &= ~((t0 < ZERO) | (t0 > ONE))
        q = R._cross(t, e0)
        t1 = R._dot(d, q) * inv_det
        ok &= ~((t1 < ZERO) | (t1 > ONE))
        t_cam = R._dot(e1, q) * inv_det
        ok &= ~((t_cam <= R.TNEAR) | (t_cam >= tfar))
        return ok, t_cam.astype(np.float32), (t0 * pl["l0"]).astype(np.float32), (t1 * pl["l1"]).astype(np.float32)


def _discrete_mis(types, L, ids, sigma_s, p_hit, p_light, rd):
    """R.discrete_mis_weights with one plane per ray."""
    with np.errstate(all="ignore"):
        d = (p_hit - p_light).astype(np.float32)
        t_sampled = R._mag(d)
        d = (d / _col(t_sampled)).astype(np.float32)
        em, lu, lv = L.emission[ids], L.u[ids], L.v[ids]
        c_uv = R._avg(R.contrib((PI * em) / sigma_s[None, :], lu, lv, rd))
        c_ut = R._avg(R.contrib(_col(PI * L.v_l[ids]) * em, lu, d, rd))
        c_vt = R._avg(R.contrib(_col(PI * L.u_l[ids]) * em, lv, d, rd))
        inv = [np.where((c != ZERO) & np.isfinite(c), ONE / c, ZERO).astype(np.float32) for c in (c_uv, c_ut, c_vt)]
        own = np.where(types == UV, c_uv, np.where(types == UT, c_ut, c_vt)).astype(np.float32)
        w = (ONE / own) / ((inv[0] + inv[1]) + inv[2])
        return np.where(np.isfinite(w), w, ZERO).astype(np.float32)


# ---- one block
def block_rect(sd, b):
    nby = (sd.height + 15) // 16
    bx, by = (b // nby) * 16, (b % nby) * 16
    return bx, by, min(16, sd.width - bx), min(16, sd.height - by)


def _resolve(draws, n_samples, nb, strategy, need):
    """Where every pair's draws sit once the redraws are placed: (jitter index [n_samples], first index [n_samples, nb], extra tries [n_samples, nb]).
    `draws(n)` gives the stream's first n draws."""
    per, pre = draws_per_plane(strategy), (2 if picks_type(strategy) else 1)
    d_s = 2 + nb * per
    base = (np.arange(n_samples, dtype=np.int64) * d_s)[:, None] + 2 + np.arange(nb, dtype=np.int64)[None, :] * per
    extra = np.zeros((n_samples, nb), np.int64)
    while True:
        before = 2 * (np.cumsum(extra.reshape(-1)) - extra.reshape(-1)).reshape(n_samples, nb)      # the extra draws of every earlier pair
        first = base + before
        s = draws(need + 2 * int(extra.sum()) + 2)
        at = (first + pre + 2 * extra).reshape(-1)
        z = _hemisphere(s[at], s[at + 1])[:, 2]
        bad = np.flatnonzero(z == ZERO)
        if bad.size == 0:
            return first[:, 0] - 2, first, extra
        extra.reshape(-1)[bad[0]] += 1


def render_block(sc, sd, lights, b, seed, nb_primitive, strategy, spp, seed_variant=0):
    """One block: dict of px, py [pixels], rgb [pixels, 3], the counters, the redraws [(lane, sample, plane)], the rays and the id_emitters used."""
    bx, by, bw, bh = block_rect(sd, b)
    L = lights
    n_pix, nb = bw * bh, nb_primitive
    n_samples = n_pix * spp
    need = n_samples * draws_per_sample(nb, strategy)
    cache = {"n": 0, "s": None}

    def draws(n):
        if n > cache["n"]:
            cache["n"], cache["s"] = n + 64, stream(seed, seed_variant, n + 64)
        return cache["s"]

    jitter, first, extra = _resolve(draws, n_samples, nb, strategy, need)
    s = draws(need + 2 * int(extra.sum()) + 2)
    lane = np.arange(n_samples) // spp
    ix, iy = lane // bh, lane % bh
    u = (bx + ix).astype(np.float32) + s[jitter]
    v = (by + iy).astype(np.float32) + s[jitter + 1]
    rays = [sc.camera_generate(float(a), float(c)) for a, c in zip(u, v)]
    o = np.asarray([r[0] for r in rays], np.float32).reshape(-1, 3)
    d = np.asarray([r[1] for r in rays], np.float32).reshape(-1, 3)
    t, _, _, mesh, _ = sc.trace(o, d)
    tfar = np.where(mesh >= 0, t, F32_MAX).astype(np.float32)

    sigma_s, sigma_t = R._v(sd.medium.sigma_s), R.sigma_t_of(sd.medium)
    at = first.reshape(-1)
    ids = np.minimum((s[at] * F32(L.n)).astype(np.int64), L.n - 1)
    if picks_type(strategy):
        pt = s[at + 1]
        types = np.where(pt < F32(1.0) / F32(3.0), UV, np.where(pt < F32(2.0) / F32(3.0), VT, UT))
        at = at + 2
    else:
        types = np.full(at.shape[0], SINGLE_TYPE[strategy])
        at = at + 1
    at = at + 2 * extra.reshape(-1)
    d_out = _hemisphere(s[at], s[at + 1])
    assert (d_out[:, 2] != ZERO).all()
    with np.errstate(all="ignore"):
        d_w = ((L.fx[ids] * _col(d_out[:, 0]) + L.fy[ids] * _col(d_out[:, 1])) + L.normal[ids] * _col(d_out[:, 2])).astype(np.float32)
        xi = s[at + 2]
        comp = (xi * F32(3.0)).astype(np.int64)
        xi = xi * F32(3.0) - comp.astype(np.float32)
        t_sampled = (-R._ln(ONE - xi) / sigma_t[np.minimum(comp, 2)]).astype(np.float32)
    sample = np.stack([s[at + 3], s[at + 4]], axis=-1)
    planes = _make_planes(L, ids, types, d_w, sample, s[at + 5], t_sampled, sigma_s)
    ray = np.repeat(np.arange(n_samples), nb)
    ok, t_cam, t0, t1 = _intersect(planes, o[ray], d[ray], tfar[ray])
    hit = np.flatnonzero(ok)
    cs = np.zeros((n_samples, 3), np.float32)
    n_visible = 0
    if hit.size:
        h_ray, h_ids, h_types = ray[hit], ids[hit], types[hit]
        rd, tc = d[h_ray], t_cam[hit]
        with np.errstate(all="ignore"):
            p_hit = (o[h_ray] + rd * _col(tc)).astype(np.float32)
            on_light = (L.o[h_ids] + L.u[h_ids] * _col(t0[hit]) + L.v[h_ids] * _col(t1[hit])).astype(np.float32)
            on_plane = (planes["o"][hit] + planes["d0"][hit] * _col(t0[hit])).astype(np.float32)
            p_light = np.where(_col(h_types == UV), on_light, on_plane).astype(np.float32)
        vis = sc.visible(p_hit, p_light).astype(bool)
        n_visible = int(vis.sum())
        k = hit[vis]
        h_ray, h_ids, h_types, rd, tc, p_hit, p_light = h_ray[vis], h_ids[vis], h_types[vis], rd[vis], tc[vis], p_hit[vis], p_light[vis]
        weight, d0, d1 = planes["weight"][k], planes["d0"][k], planes["d1"][k]
        with np.errstate(all="ignore"):
            tau = np.where(_col(np.isfinite(tc)), sigma_t[None, :] * _col(tc), ZERO).astype(np.float32)
            trans = _expf(-tau)
            if strategy == "average":
                w = np.full(k.shape[0], ONE / F32(3.0), np.float32)
            elif strategy == "discrete_mis":
                w = _discrete_mis(h_types, L, h_ids, sigma_s, p_hit, p_light, rd)
            else:
                w = np.ones(k.shape[0], np.float32)
            if strategy == "cmis":
                a = R._dot(R._cross(L.u[h_ids], d1), rd)
                bb = R._dot(R._cross(L.v[h_ids], d1), rd)
                flux = _col((ONE / ((F32(2.0) / PI) * np.sqrt(a * a + bb * bb))).astype(np.float32)) * weight
            else:
                flux = R.contrib(weight, d0, d1, rd)
            rho = ONE / (PI * F32(4.0))
            val = ((((_col(w * rho) * trans) * sigma_s[None, :]) * flux) * F32(L.n) * (ONE / F32(nb))).astype(np.float32)
        # c += ..., plane after plane: the k-th visible plane of every sample in pass k
        starts = np.flatnonzero(np.r_[True, h_ray[1:] != h_ray[:-1]])
        rank = np.arange(h_ray.shape[0]) - np.repeat(starts, np.diff(np.r_[starts, h_ray.shape[0]]))
        for r in range(int(rank.max()) + 1 if rank.size else 0):
            m = rank == r
            cs[h_ray[m]] = cs[h_ray[m]] + val[m]
    acc = np.zeros((n_pix, 3), np.float32)
    for k in range(spp):                                   # im_block.accumulate in sample order
        acc = acc + cs[k::spp]
    rgb = acc * (ONE / F32(spp))                           # im_block.scale(1.0 / nb_samples as f32)
    where = np.argwhere(extra > 0)
    redraws = [(int(si) // spp, int(si) % spp, int(j)) for si, j in where for _ in range(int(extra[si, j]))]
    pix_lane = np.arange(n_pix)
    corners_finite = True
    with np.errstate(all="ignore"):
        e0, e1 = planes["d0"] * _col(planes["l0"]), planes["d1"] * _col(planes["l1"])
        corners_finite = bool(np.isfinite(planes["o"]).all() and np.isfinite(planes["o"] + e0).all() and np.isfinite(planes["o"] + e1).all()
                              and np.isfinite(planes["o"] + e0 + e1).all())
    return {"px": bx + pix_lane // bh, "py": by + pix_lane % bh, "rgb": rgb.astype(np.float32), "samples": n_samples, "redraws": redraws,
            "draws": need + 2 * len(redraws), "intersected": int(hit.size), "visible": n_visible, "o": o, "d": d, "tfar": tfar, "ids": set(int(i) for i in np.unique(ids)),
            "corners_finite": corners_finite}


def render(sc, sd, seeds, nb_primitive, strategy, spp=1, seed_variant=0, shard_index=0, shard_count=1):
    """(image HxWx3 f32, the counters rl_render_plane_uncorrelated reports, detail).  detail: per block the lanes that drew again ("redraw_lanes": {block:
    [(lane, sample, plane)]}), the rays ("blocks": {block: render_block's dict}), the id_emitters used, whether every plane corner is finite."""
    L = _Lights(R.rect_lights(sd))
    img = np.zeros((sd.height, sd.width, 3), np.float32)
    st = {"camera_samples": 0, "extension_rays": 0, "shadow_rays": 0, "rng_draws": 0, "redraws": 0, "planes_intersected": 0, "planes_visible": 0}
    detail = {"redraw_lanes": {}, "blocks": {}, "ids": set(), "corners_finite": True}
    for b, seed in enumerate(np.asarray(seeds, np.uint64)):
        if b % shard_count != shard_index:
            continue
        r = render_block(sc, sd, L, b, int(seed), nb_primitive, strategy, spp, seed_variant)
        img[r["py"], r["px"]] = r["rgb"]
        st["camera_samples"] += r["samples"]
        st["rng_draws"] += r["draws"]
        st["redraws"] += len(r["redraws"])
        st["planes_intersected"] += r["intersected"]
        st["planes_visible"] += r["visible"]
        if r["redraws"]:
            detail["redraw_lanes"][b] = r["redraws"]
        detail["blocks"][b] = r
        detail["ids"] |= r["ids"]
        detail["corners_finite"] &= r["corners_finite"]
    st["extension_rays"], st["shadow_rays"] = st["camera_samples"], st["planes_intersected"]
    return img, st, detail


def compute(sd, seed=0, nb_primitive=128, strategy="average", spp=1, seed_variant=0):
    """IntegratorSinglePlaneUncorrelated::compute seed for seed: the block seeds straight from the main sampler seeded as `-r independent:SEED` (:83)."""
    sc = orc.Scene(sd)
    seeds = orc.block_seeds(seed, sd.width, sd.height, seed_variant)
    img, st, detail = render(sc, sd, seeds, nb_primitive, strategy, spp, seed_variant)
    return {"seeds": seeds, "image": img, "stats": st, "detail": detail, "scene": sc}


# ---- the literal scalar walk of one block
def walk_block(sc, sd, b, seed, nb_primitive, strategy, spp, seed_variant=0):
    """The reference's loop, draw after draw on one orc.Rng, with plane_single_restatement's own pieces: render_block's dict without the rays."""
    lights = R.rect_lights(sd)
    sigma_s, sigma_t = R._v(sd.medium.sigma_s), R.sigma_t_of(sd.medium)
    bx, by, bw, bh = block_rect(sd, b)
    rng = orc.Rng(int(seed), seed_variant)
    count = {"draws": 0}

    def nxt():
        count["draws"] += 1
        return F32(rng.next_f32())

    rgb = np.zeros((bw * bh, 3), np.float32)
    redraws, n_isect, n_vis, n_samples = [], 0, 0, 0
    rho = ONE / (PI * F32(4.0))
    for ix in range(bw):
        for iy in range(bh):
            acc = np.zeros(3, np.float32)
            for smp in range(spp):
                n_samples += 1
                u = F32(bx + ix) + nxt()
                v = F32(by + iy) + nxt()
                o, d = sc.camera_generate(float(u), float(v))
                o, d = R._v(o).reshape(1, 3), R._v(d).reshape(1, 3)
                t, _, _, mesh, _ = sc.trace(o, d)
                tfar = np.where(mesh >= 0, t, F32_MAX).astype(np.float32)
                c = np.zeros(3, np.float32)
                for j in range(nb_primitive):
                    id_emitter = min(int(nxt() * F32(len(lights))), len(lights) - 1)
                    light = lights[id_emitter]
                    if picks_type(strategy):
                        plane_type = nxt()
                        kind = UV if plane_type < F32(1.0) / F32(3.0) else (VT if plane_type < F32(2.0) / F32(3.0) else UT)
                    else:
                        kind = SINGLE_TYPE[strategy]
                    d_out = R.cosine_sample_hemisphere(nxt(), nxt())
                    while d_out[2] == ZERO:
                        redraws.append((ix * bh + iy, smp, j))
                        d_out = R.cosine_sample_hemisphere(nxt(), nxt())
                    d_w = R.frame_to_world(light.n, d_out)
                    xi = nxt()
                    component = int(xi * F32(3.0))
                    xi = xi * F32(3.0) - F32(component)
                    with np.errstate(all="ignore"):
                        t_sampled = -R._ln(ONE - xi) / sigma_t[min(component, 2)]
                    sample = (nxt(), nxt())
                    pl = R.plane_new(kind, light, d_w, sample, nxt(), t_sampled, id_emitter, sigma_s)
                    ok, t_cam, t0, t1 = R.intersect(pl, o, d, tfar)
                    if not ok[0]:
                        continue
                    n_isect += 1
                    with np.errstate(all="ignore"):
                        p_hit = (o + d * t_cam[:, None]).astype(np.float32)
                    p_light = R.light_position(pl, light, t0, t1)
                    if not sc.visible(p_hit, p_light)[0]:
                        continue
                    n_vis += 1
                    with np.errstate(all="ignore"):
                        tau = np.where(np.isfinite(t_cam)[:, None], sigma_t[None, :] * t_cam[:, None], ZERO).astype(np.float32)
                        trans = _expf(-tau)
                        if strategy == "average":
                            w = np.full(1, ONE / F32(3.0), np.float32)
                        elif strategy == "discrete_mis":
                            w = R.discrete_mis_weights(pl, light, sigma_s, p_hit, p_light, d)
                        else:
                            w = np.ones(1, np.float32)
                        flux = R.w_cmis(pl, light, d)[:, None] * pl.weight[None, :] if strategy == "cmis" else R.contrib(pl.weight, pl.d0, pl.d1, d)
                        val = ((((w * rho)[:, None] * trans) * sigma_s[None, :]) * flux).astype(np.float32)
                        c = c + (val[0] * F32(len(lights)) * (ONE / F32(nb_primitive))).astype(np.float32)
                acc = acc + c
            rgb[ix * bh + iy] = acc * (ONE / F32(spp))
    lane = np.arange(bw * bh)
    return {"px": bx + lane // bh, "py": by + lane % bh, "rgb": rgb, "samples": n_samples, "redraws": redraws, "draws": count["draws"], "intersected": n_isect,
            "visible": n_vis}


# ---- the camera rays alone, for the quadrature (tests/test_gpu_uplane_quadrature.py)
def zero_redraws(zeros, pair_at, nb_primitive, strategy):
    """The redraws of a block found from the draws that are exactly 0.0 (`zeros`, their indices in the stream, ascending) — a direction has z == 0 only with
    such a coordinate, which tests/test_uplane_restatement.py holds against _resolve on the redraw cases.  pair_at(i) = draws i and i + 1.  [(sample, plane)]
    in stream order."""
    per, pre = draws_per_plane(strategy), (2 if picks_type(strategy) else 1)
    d_s = 2 + nb_primitive * per
    out, shift, done = [], 0, -1
    for i in zeros:
        i = int(i)
        if i <= done:
            continue
        smp, r = divmod(i - shift, d_s)
        if r < 2:
            continue
        j, k = divmod(r - 2, per)
        if k not in (pre, pre + 1):
            continue
        at = i - (k - pre)
        while True:
            ux, uy = pair_at(at)
            if _hemisphere(np.asarray([ux], np.float32), np.asarray([uy], np.float32))[0, 2] != ZERO:
                break
            out.append((smp, j))
            shift, at = shift + 2, at + 2
        done = at + 1
    return out


def camera_rays(sc, sd, seeds, nb_primitive, strategy, seed_variant=0, zeros_of=zero_draws):
    """(pixel x, pixel y, o, d, tfar, redraws) of every camera sample at 1 spp: lane c's jitter sits at draws c D and c D + 1 of its block's stream, plus 2 per
    direction drawn again before it.  Nothing but the jitter is evaluated: the redraws are found from the stream's exact zeros (zero_redraws); zeros_of(seed,
    variant, n) gives their indices below n (a caller that asks for several plane layouts of one stream may keep them)."""
    d_s = draws_per_sample(nb_primitive, strategy)
    px, py, os_, ds, n_redraws = [], [], [], [], 0
    for b, seed in enumerate(np.asarray(seeds, np.uint64)):
        bx, by, bw, bh = block_rect(sd, b)
        shift = np.zeros(bw * bh, np.int64)
        zeros = zeros_of(int(seed), seed_variant, bw * bh * d_s)
        for smp, _ in zero_redraws(zeros, lambda i: draws_at(int(seed), seed_variant, i, 2), nb_primitive, strategy):
            shift[smp + 1:] += 2
            n_redraws += 1
        step = _jump_matrix(d_s)
        bits = _state_bits(int(seed), seed_variant)
        for c in range(bw * bh):
            ix, iy = c // bh, c % bh
            st = bits if shift[c] == 0 else np.mod(_jump_matrix(int(shift[c])) @ bits, 2.0)
            r = orc.Rng.from_state([int(v) for v in _unbits(st)[:, 0]])
            o, d = sc.camera_generate(float(F32(bx + ix) + F32(r.next_f32())), float(F32(by + iy) + F32(r.next_f32())))
            px.append(bx + ix); py.append(by + iy); os_.append(o); ds.append(d)
            bits = np.mod(step @ bits, 2.0)
    o, d = np.asarray(os_, np.float32).reshape(-1, 3), np.asarray(ds, np.float32).reshape(-1, 3)
    t, _, _, mesh, _ = sc.trace(o, d)
    return np.asarray(px), np.asarray(py), o, d, np.where(mesh >= 0, t, F32_MAX).astype(np.float32), n_redraws


# ---- the fixtures the CPU and the GPU tests share, each computed once and left unchanged
_CACHE = {}


def fixture(strategy):
    """cbox_medium(32, 24, 1.0), seed 3, spp 2, FIXTURE_NB[strategy] planes: (sd, seeds, nb_primitive, spp, image, stats, detail)."""
    if strategy not in _CACHE:
        from rustlight_amd import scenes
        sd = scenes.cbox_medium(32, 24, 1.0)
        seeds = orc.block_seeds(3, 32, 24)
        _CACHE[strategy] = (sd, seeds, FIXTURE_NB[strategy], 2) + render(orc.Scene(sd), sd, seeds, FIXTURE_NB[strategy], strategy, 2)
    return _CACHE[strategy]


def redraw_case(i):
    """REDRAW_CASES[i] on a 32 x 24 frame: its seed goes to block 0 (even i) or block 2 (odd i), both full 16 x 16 blocks, the other blocks take
    orc.block_seeds(3, ..).  (sd, seeds, block, case, image, stats, detail)."""
    if ("redraw", i) not in _CACHE:
        from rustlight_amd import scenes
        seed, strategy, nb, spp = REDRAW_CASES[i][:4]
        sd = scenes.cbox_medium(32, 24, 1.0)
        seeds = orc.block_seeds(3, 32, 24).copy()
        block = 2 * (i % 2)
        seeds[block] = seed
        _CACHE[("redraw", i)] = (sd, seeds, block, REDRAW_CASES[i]) + render(orc.Scene(sd), sd, seeds, nb, strategy, spp)
    return _CACHE[("redraw", i)]
