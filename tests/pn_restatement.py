"""IntegratorPointNormal's seven plain strategies restated in float32 numpy from the reference's text (src/integrators/explicit/point_normal.rs), the yardstick
of tests/test_pn_restatement.py, tests/test_gpu_pn_exact.py, tests/test_gpu_pn_fuzz.py and tests/test_gpu_pn_quadrature.py (a plain module: `from tests import
pn_restatement`).

compute_pixel (:2585-2633, use_mis = false, splitting = None): 2 draws for the pixel jitter (none with AA off: the pixel centre), camera.generate, accel.trace
for max_dist; then compute_single_tr (:2209-2284), compute_single_tr_phase (:2287-2334) or compute_single_strategy (:2336-2453) with
create_distance_sampling's three plain arms (:1393, :1547, :1550), EquiAngularSampling::{new, new_clamping, sample} (:26-166), PointNormalSampling::{new,
sample} (:660-739), TransmittanceSampling::sample (:1087-1116) and fix_random_sample_emitter's non-ATS arm (:1201-1216) with
EmitterSampler::random_sample_emitter_position (emitter.rs:1752-1762), Mesh::sample / sample_tri (geometry.rs:261-348), Distribution1DConstruct::normalize
(math.rs:418-441) and PhaseFunction / HomogenousVolume (volume.rs).

Draws per camera sample after the jitter's 2:   tr_ex 1 distance + 4 emitter (next, next, next2d) | tr_phase 1 + 2 phase | eq_ex 4 + 1 | eq_phase 4 + 1 + 2 |
eq_clamped_ex, pn_ex 4, then 1 only when a distance sampler exists | eq_clamped_phase 4, then 3 only then.

Defined where the reference panics, as the kernel defines it: (1) EquiAngularSampling::new's assert!(theta_a < theta_b) (:42) — the sample takes its usual
draws and adds zero; (2) TransmittanceSampling's panic when the distance `exited` on an unbounded ray (:1093-1096) — the same.  Everything else is literal:
Color / f32 and Color * f32 guard their scalar, f32::max ignores NaN (np.fmax), signum(+-0) = +-1 (np.copysign), crate::clamp lets NaN through, theta_b =
FRAC_PI_2 - 0.00001 on a miss.  atan(x) = atan2f_det(x, 1), tan = sinf_det / cosf_det, powi(2) = x * x.

Every float operation is a float32 elementwise numpy operation in the reference's order (dot = (x x' + y y') + z z', nothing fused) over arrays of camera
samples.  Two forms over the same elementwise statements: walk_block is the literal scalar loop — one orc.Rng per block, one camera sample at a time (arrays
of one element), every draw taken where the reference takes it; render has every sample of the frame as one array element, its draws read from the block's
stream (a numpy xoshiro256++, tests/uplane_restatement.stream) at the sample's offset.  For the three data-dependent strategies the offsets come from a walk
of the None test alone (chain_offsets), which is what the device's chain pass does.  Camera ray, trace, trace_full, visible, orc.Rng, orc.block_seeds and the
math (sin, cos, exp, log, atan2 through orc_math_batch) are the oracle's."""

import numpy as np

from oracle import orc
from rustlight_amd import abi, api
from tests import plane_single_restatement as R
from tests import uplane_restatement as U
from tests.bre_restatement import F32, F32_MAX, _expf

STRATEGIES = api.PN_STRATEGIES
PI, FRAC_PI_2, FRAC_1_PI, ONE, ZERO = F32(np.pi), F32(np.pi / 2), F32(1.0 / np.pi), F32(1.0), F32(0.0)
COUNTERS = ("camera_samples", "rng_draws", "extension_rays", "shadow_rays", "vertices")
RL_ERR_INVALID_ARGUMENT, RL_ERR_UNSUPPORTED, RL_ERR_NO_EMITTER = -1, -7, -8


class Refused(Exception):
    def __init__(self, code, why):
        super().__init__(why)
        self.code = code


def is_tr(s):
    return s in ("tr_ex", "tr_phase")


def is_phase(s):
    return s.endswith("_phase")


def may_fail(s):
    return s in ("eq_clamped_ex", "eq_clamped_phase", "pn_ex")


def draws_per_sample(strategy, use_aa=True):
    """The constant count D of a strategy, None when it depends on the data."""
    base = {"tr_ex": 5, "tr_phase": 3, "eq_ex": 5, "eq_phase": 7}.get(strategy)
    return None if base is None else base + (2 if use_aa else 0)


def max_draws(strategy, use_aa=True):
    return (2 if use_aa else 0) + {"tr_ex": 5, "tr_phase": 3, "eq_ex": 5, "eq_phase": 7, "eq_clamped_ex": 5, "pn_ex": 5, "eq_clamped_phase": 7}[strategy]


# ---- the float32 pieces
def _math2(fn, a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(np.broadcast_to(np.asarray(b, np.float32), a.shape), np.float32)
    out = np.zeros_like(a)
    if a.size:
        orc.lib().orc_math_batch(fn, a.size, abi.fptr(a.reshape(-1)), abi.fptr(b.reshape(-1)), abi.fptr(out.reshape(-1)))
    return out


def _sin(x):
    return _math2(0, x, x)


def _cos(x):
    return _math2(1, x, x)


def _ln(x):
    return _math2(3, x, x)


def _atan2(y, x):
    return _math2(6, y, x)


def _atan(x):
    return _atan2(x, ONE)


def _tan(x):
    return (_sin(x) / _cos(x)).astype(np.float32)


def _col(a):
    return a[:, None]


def _mul_guarded(c, s):
    """Color * f32 (structure.rs): a non-finite factor gives black.  c [n, 3] or [3], s [n]."""
    s = np.asarray(s, np.float32)
    return np.where(_col(np.isfinite(s)), c * _col(s), ZERO).astype(np.float32)


def _normalize(a):
    """cgmath normalize: v * (1 / |v|)."""
    return (a * _col(ONE / R._mag(a))).astype(np.float32)


def build_cdf(elements):
    """Distribution1DConstruct::normalize (math.rs:418-441): (cdf [n + 1] f32, func_int)."""
    elements = np.asarray(elements, np.float32)
    n = F32(len(elements))
    cdf, cur = [], F32(0.0)
    for e in elements:
        cdf.append(cur)
        cur = F32(cur + F32(e / n))
    cdf.append(cur)
    cdf = np.asarray(cdf, np.float32)
    if cur != 0.0:
        cdf = (cdf / cur).astype(np.float32)
    cdf[-1] = ONE
    return cdf, cur


def sample_discrete(cdf, v):
    """Distribution1D::sample_discrete (math.rs:447-457) for distinct cdf entries: the last index whose entry is <= v."""
    return np.maximum(np.searchsorted(cdf, v, side="right") - 1, 0)


class Emitters:
    """EmitterSampler of a scene without the light tree (scene.rs:60-117): the emissive meshes in mesh order, then the point lights."""

    def __init__(self, sd):
        self.kind, self.mesh, self.position, self.intensity = [], [], [], []
        flux = []
        for m in sd.meshes:
            if m.emission is None:
                continue
            assert m.emission_kind is None, "constant emission only"
            v = R._v(m.vertices).reshape(-1, 3)
            idx = np.asarray(m.indices).reshape(-1, 3)
            v0, v1, v2 = v[idx[:, 0]], v[idx[:, 1]], v[idx[:, 2]]
            area = (R._mag(R._cross(v1 - v0, v2 - v0)) * F32(0.5)).astype(np.float32)          # Mesh::new (geometry.rs:130-138)
            cdf, func_int = build_cdf(area)
            total = F32(func_int * F32(len(area)))                                            # Distribution1D::total (math.rs:484-486)
            normals = None
            if m.normals is not None:                                                        # Mesh::new normalises them (geometry.rs:143-153)
                normals = R._v(m.normals).reshape(-1, 3).copy()
                l = R._dot(normals, normals)
                fix = (l != ZERO) & (l != ONE)
                with np.errstate(all="ignore"):
                    normals[fix] = (normals[fix] / _col(np.sqrt(l[fix]))).astype(np.float32)
            e = R._v(m.emission)
            self.kind.append("mesh")
            self.mesh.append({"v": v, "idx": idx, "normals": normals, "cdf": cdf, "total": total, "emission": e})
            self.position.append(None); self.intensity.append(None)
            flux.append(np.max(((e * total) * PI).astype(np.float32)))                         # Mesh::flux (emitter.rs:591-599), channel_max
        for lt in sd.lights:
            assert lt["type"] == "point"
            c = R._v(lt["intensity"])
            self.kind.append("point"); self.mesh.append(None)
            self.position.append(R._v(lt["a"])); self.intensity.append(c)
            flux.append(np.max(((c * F32(4.0)) * PI).astype(np.float32)))                      # PointEmitter::flux (emitter.rs:239-241)
        self.n = len(self.kind)
        self.cdf, _ = build_cdf(flux) if self.n else (None, None)

    def sample(self, r_sel, r_pos, ux, uy):
        """random_sample_emitter_position then * correct_flux(): (p [n, 3], n [n, 3], flux [n, 3], is_surface [n])."""
        n = r_sel.shape[0]
        ids = sample_discrete(self.cdf, r_sel)
        pdf_sel = (self.cdf[ids + 1] - self.cdf[ids]).astype(np.float32)
        p, nrm, flux = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        surface = np.zeros(n, bool)
        correct = np.zeros(n, np.float32)
        with np.errstate(all="ignore"):
            for e in range(self.n):
                m = ids == e
                if not m.any():
                    continue
                if self.kind[e] == "point":                                                  # PointEmitter::sample_position (emitter.rs:217-229)
                    p[m] = self.position[e]
                    flux[m] = ((self.intensity[e] * F32(4.0)) * PI).astype(np.float32)
                    correct[m] = ONE / (F32(4.0) * PI)
                    continue
                me = self.mesh[e]
                prim = sample_discrete(me["cdf"], r_pos[m])                                  # Mesh::sample (geometry.rs:340-348)
                i0, i1, i2 = me["idx"][prim, 0], me["idx"][prim, 1], me["idx"][prim, 2]
                v0, v1, v2 = me["v"][i0], me["v"][i1], me["v"][i2]
                su0 = np.sqrt(ux[m]).astype(np.float32)                                      # uniform_sample_triangle (math.rs:388-394)
                b0, b1 = (ONE - su0).astype(np.float32), (uy[m] * su0).astype(np.float32)
                b2 = ((ONE - b0) - b1).astype(np.float32)
                p[m] = ((v0 * _col(b0) + v1 * _col(b1)) + v2 * _col(b2)).astype(np.float32)
                n_g = _normalize(R._cross(v2 - v0, v1 - v0))
                if me["normals"] is not None:
                    n0, n1, n2 = me["normals"][i0], me["normals"][i1], me["normals"][i2]
                    ns = ((n0 * _col(b0) + n1 * _col(b1)) + n2 * _col(b2)).astype(np.float32)
                    n_l = R._dot(ns, ns)
                    ns = np.where(_col(n_l == ZERO), n_g, np.where(_col(n_l != ONE), ns / _col(np.sqrt(n_l)), ns)).astype(np.float32)
                    n_g = np.where(_col(R._dot(n_g, ns) < ZERO), -n_g, n_g).astype(np.float32)
                nrm[m] = n_g
                surface[m] = True
                flux[m] = ((me["emission"] * PI) / (ONE / me["total"])).astype(np.float32)   # emit * PI / pdf.value(), pdf = Area(1 / cdf.total())
                correct[m] = ONE / PI
            flux = (flux / _col(pdf_sel)).astype(np.float32)                                 # w / pdf_sel
            flux = _mul_guarded(flux, correct)
        return p, nrm, flux, surface


class Medium:
    def __init__(self, med):
        self.sigma_s = R._v(med.sigma_s)
        self.sigma_t = (R._v(med.sigma_a) + R._v(med.sigma_s)).astype(np.float32)
        self.hg = med.phase != 0
        self.g = F32(med.g)

    def transmittance(self, t):
        return _expf(-_mul_guarded(self.sigma_t[None, :], t))

    def phase_eval(self, w_i, w_o):
        n = w_i.shape[0]
        if not self.hg:
            return np.full((n, 3), ONE / (PI * F32(4.0)), np.float32)
        g = self.g
        with np.errstate(all="ignore"):
            tmp = ((ONE + g * g) + (F32(2.0) * g) * R._dot(w_i, w_o)).astype(np.float32)
            val = (((FRAC_1_PI * F32(0.25)) * (ONE - g * g)) / (tmp * np.sqrt(tmp))).astype(np.float32)
        return np.repeat(_col(val), 3, axis=1)

    def phase_sample(self, d_in, ux, uy):
        """PhaseFunction::sample (volume.rs:34-67): the direction (the weight is one)."""
        with np.errstate(all="ignore"):
            phi = ((F32(2.0) * PI) * uy).astype(np.float32)
            if not self.hg:                                                                  # sample_uniform_sphere
                z = (ONE - F32(2.0) * ux).astype(np.float32)
                r = np.sqrt(np.fmax(ONE - z * z, ZERO)).astype(np.float32)
                return np.stack([r * _cos(phi), r * _sin(phi), z], axis=-1).astype(np.float32)
            g = self.g
            if abs(g) < F32(0.000001):
                cos_t = (ONE - F32(2.0) * ux).astype(np.float32)
            else:
                sq = ((ONE - g * g) / ((ONE - g) + (F32(2.0) * g) * ux)).astype(np.float32)
                cos_t = (((ONE + g * g) - sq * sq) / (F32(2.0) * g)).astype(np.float32)
            sin_t = np.sqrt(np.fmax(ONE - cos_t * cos_t, ZERO)).astype(np.float32)
            sp, cp = _sin(phi), _cos(phi)
            nz = (d_in * F32(-1.0)).astype(np.float32)                                       # Frame::new(d_in_reverse)
            sign = np.copysign(ONE, nz[:, 2]).astype(np.float32)
            a = (F32(-1.0) / (sign + nz[:, 2])).astype(np.float32)
            b = ((nz[:, 0] * nz[:, 1]) * a).astype(np.float32)
            fx = np.stack([ONE + ((sign * nz[:, 0]) * nz[:, 0]) * a, sign * b, -sign * nz[:, 0]], axis=-1).astype(np.float32)
            fy = np.stack([b, sign + (nz[:, 1] * nz[:, 1]) * a, -nz[:, 1]], axis=-1).astype(np.float32)
            return ((fx * _col(sin_t * cp) + fy * _col(sin_t * sp)) + nz * _col(cos_t)).astype(np.float32)


# ---- the distance samplers
def make_sampler(strategy, has_max, max_dist, o, d, pos, nrm):
    """create_distance_sampling's plain arms for the equi-angular family: (sampler dict, ok [n]); ok false = None, or defined panic (1) for eq_ex / eq_phase."""
    with np.errstate(all="ignore"):
        delta = R._dot(d, (pos - o).astype(np.float32)).astype(np.float32)
        d_l = R._mag((pos - (o + d * _col(delta))).astype(np.float32))
        theta_a = _atan((-delta / d_l).astype(np.float32))
        theta_b = np.where(has_max, _atan(((max_dist - delta) / d_l).astype(np.float32)), FRAC_PI_2 - F32(0.00001)).astype(np.float32)
        s = {"delta": delta, "d_l": d_l, "theta_a": theta_a, "theta_b": theta_b, "a": np.zeros_like(delta), "b": np.zeros_like(delta)}
        if not may_fail(strategy):
            return s, theta_a < theta_b
        d_dot_n = R._dot(d, nrm).astype(np.float32)
        p_dot_n = R._dot((pos - o).astype(np.float32), nrm).astype(np.float32)
        none = (d_dot_n <= ZERO) & (p_dot_n >= ZERO)
        unclamped = (np.abs(d_dot_n) < F32(0.00001)) | ((p_dot_n == ZERO) & (d_dot_n > ZERO))
        t_hit = (p_dot_n / d_dot_n).astype(np.float32)
        outside = (t_hit < ZERO) | (t_hit > np.where(has_max, max_dist, F32_MAX))
        alpha = _atan(((t_hit - delta) / d_l).astype(np.float32))
        clamp = ~unclamped & ~outside
        behind = p_dot_n > ZERO
        theta_a = np.where(clamp & behind, alpha, theta_a).astype(np.float32)
        theta_b = np.where(clamp & ~behind, alpha, theta_b).astype(np.float32)
        s["theta_a"], s["theta_b"] = theta_a, theta_b
        ok = ~none & ~(theta_a >= theta_b)
        if strategy != "pn_ex":
            return s, ok
        ok &= ~(theta_b <= theta_a)
        dv = (((o + d * _col(delta)) - pos) / _col(d_l)).astype(np.float32)
        a, b = R._dot(nrm, dv).astype(np.float32), R._dot(nrm, d).astype(np.float32)
        norm = (a * (_sin(theta_b) - _sin(theta_a)) - b * (_cos(theta_b) - _cos(theta_a))).astype(np.float32)
        s["a"], s["b"] = (a / norm).astype(np.float32), (b / norm).astype(np.float32)
        return s, ok & ~(norm <= ZERO)


def sample_equiangular(s, has_max, max_dist, xi):
    with np.errstate(all="ignore"):
        t = (s["d_l"] * _tan(((ONE - xi) * s["theta_a"] + xi * s["theta_b"]).astype(np.float32))).astype(np.float32)
        t_eq = (t + s["delta"]).astype(np.float32)
        pdf = ((s["theta_b"] - s["theta_a"]) * (s["d_l"] * s["d_l"] + t * t)).astype(np.float32)
        pdf = np.where(pdf != ZERO, s["d_l"] / pdf, pdf).astype(np.float32)
        t_eq = np.where(t_eq < ZERO, ZERO, t_eq)
        t_eq = np.where(has_max & (t_eq > max_dist), max_dist, t_eq).astype(np.float32)
    return t_eq, pdf


def sample_point_normal(s, xi):
    with np.errstate(all="ignore"):
        a, b, ta, tb = s["a"], s["b"], s["theta_a"], s["theta_b"]
        smp = ((xi + a * _sin(ta)) - b * _cos(ta)).astype(np.float32)
        v = np.sqrt(np.fmax((a * a + b * b) - smp * smp, ZERO)).astype(np.float32)
        q = (a * smp).astype(np.float32)
        r = ((b * v) / np.copysign(ONE, a)).astype(np.float32)
        r = np.where(np.isnan(a), a, r).astype(np.float32)                                   # signum(NaN) = NaN
        sv = (-b * smp).astype(np.float32)
        t = (v * np.abs(a)).astype(np.float32)
        sol1 = _atan2((q + r).astype(np.float32), (sv + t).astype(np.float32))
        theta = np.where((sol1 >= ta) & (sol1 <= tb), sol1, _atan2((q - r).astype(np.float32), (sv - t).astype(np.float32))).astype(np.float32)
        theta = np.where(theta < ta, ta, np.where(theta > tb, tb, theta)).astype(np.float32)     # crate::clamp
        sin_t, cos_t = _sin(theta), _cos(theta)
        td = (s["d_l"] * (sin_t / cos_t)).astype(np.float32)
        pdf_angular = (a * cos_t + b * sin_t).astype(np.float32)
        jacobian = (s["d_l"] / (s["d_l"] * s["d_l"] + td * td)).astype(np.float32)
        return (td + s["delta"]).astype(np.float32), np.abs(pdf_angular * jacobian).astype(np.float32)


def sample_transmittance(med, has_max, max_dist, xi):
    """TransmittanceSampling::sample: (t, pdf, ok); ok false = defined panic (2)."""
    sigma_t = med.sigma_t
    with np.errstate(all="ignore"):
        comp = np.clip((xi * F32(3.0)).astype(np.int64), 0, 255)                             # `as u8`
        u = (xi * F32(3.0) - comp.astype(np.float32)).astype(np.float32)
        sigma_t_c = sigma_t[np.minimum(comp, 2)]
        # None: HomogenousVolume::sample with tfar = f32::MAX
        t0 = (-_ln((ONE - u).astype(np.float32)) / sigma_t_c).astype(np.float32)
        tmin = np.fmin(t0, F32_MAX).astype(np.float32)
        pdf0 = R._avg((sigma_t[None, :] * _expf(-(_col(tmin) * sigma_t[None, :]).astype(np.float32))).astype(np.float32))
        # Some(v)
        norm = (ONE - _expf((-sigma_t_c * max_dist).astype(np.float32))).astype(np.float32)
        t1 = (-_ln((ONE - u * norm).astype(np.float32)) / sigma_t_c).astype(np.float32)
        norm_c = (ONE - _expf(_mul_guarded(-sigma_t[None, :], max_dist))).astype(np.float32)
        pdf1 = R._avg(((sigma_t[None, :] / norm_c) * _expf(_mul_guarded(-sigma_t[None, :], t1))).astype(np.float32))
    t = np.where(has_max, t1, tmin).astype(np.float32)
    pdf = np.where(has_max, pdf1, pdf0).astype(np.float32)
    return t, pdf, has_max | ~(t0 >= F32_MAX)


class Frame:
    """What a render needs of a scene, made once: the oracle's scene, the emitters, the medium."""

    def __init__(self, sd, sc=None):
        check_scene(sd)
        self.sd, self.sc = sd, sc or orc.Scene(sd)
        self.emitters, self.medium = Emitters(sd), Medium(sd.medium)
        self.light_mesh = {i: R._v(m.emission) for i, m in enumerate(sd.meshes) if m.emission is not None}


def check_scene(sd):
    """What rl_render_point_normal refuses about the scene, with its codes."""
    if sd.medium is None or not (np.asarray(sd.medium.sigma_a, np.float32) + np.asarray(sd.medium.sigma_s, np.float32)).any():
        raise Refused(RL_ERR_UNSUPPORTED, "no medium")
    if getattr(sd, "use_ats", False):
        raise Refused(RL_ERR_UNSUPPORTED, "light tree")
    if sd.environment is not None or sd.environment_map is not None:
        raise Refused(RL_ERR_UNSUPPORTED, "environment emitter")
    if any(lt["type"] != "point" for lt in sd.lights):
        raise Refused(RL_ERR_UNSUPPORTED, "directional light")
    if not sd.lights and not any(m.emission is not None for m in sd.meshes):
        raise Refused(RL_ERR_NO_EMITTER, "no emitter")


def check_params(strategy, spp, stream_mode, shard_index, shard_count, use_aa=True, single_pass=False):
    if spp == 0:
        raise Refused(RL_ERR_INVALID_ARGUMENT, "spp")
    if strategy not in STRATEGIES:
        raise Refused(RL_ERR_INVALID_ARGUMENT, "strategy")
    if stream_mode == api.STREAM_STRATIFIED:
        raise Refused(RL_ERR_UNSUPPORTED, "stratified")
    if stream_mode not in (api.STREAM_REFERENCE_ORDER, api.STREAM_PER_SAMPLE) or shard_index >= max(shard_count, 1):
        raise Refused(RL_ERR_INVALID_ARGUMENT, "stream mode / shard")
    d = draws_per_sample(strategy, use_aa)
    if stream_mode == api.STREAM_REFERENCE_ORDER and not single_pass and d is not None and 256 * spp * d > 0xffffffff:
        raise Refused(RL_ERR_UNSUPPORTED, "jump-ahead reach")


def evaluate(fr, strategy, use_aa, px, py, draw):
    """compute_pixel for the camera samples of pixels (px, py) [n]: draw() gives the next draw of every sample, [n] f32, and is called exactly where the
    reference draws (a walk of one sample stops drawing where that sample stops).  Returns (radiance [n, 3], counts dict of [n] arrays)."""
    n = px.shape[0]
    sc, med = fr.sc, fr.medium
    if use_aa:
        u, v = (px.astype(np.float32) + draw()).astype(np.float32), (py.astype(np.float32) + draw()).astype(np.float32)
    else:
        u, v = (px.astype(np.float32) + F32(0.5)).astype(np.float32), (py.astype(np.float32) + F32(0.5)).astype(np.float32)
    rays = [sc.camera_generate(float(a), float(b)) for a, b in zip(u, v)]
    o = np.asarray([r[0] for r in rays], np.float32).reshape(-1, 3)
    d = np.asarray([r[1] for r in rays], np.float32).reshape(-1, 3)
    t, _, _, mesh, _ = sc.trace(o, d)
    has_max, max_dist = mesh >= 0, t.astype(np.float32)
    draws = np.full(n, 2 if use_aa else 0, np.int64)
    ok = np.ones(n, bool)
    some = np.ones(n, bool)                                                                  # a distance sampler existed
    out = np.zeros((n, 3), np.float32)
    zeros = {"draws": draws, "ext": np.ones(n, np.int64), "shadow": np.zeros(n, np.int64), "vertices": np.zeros(n, np.int64), "some": some,
             "o": o, "d": d, "has_max": has_max, "max_dist": max_dist}
    pos = nrm = flux = surface = None
    if is_tr(strategy):
        t_cam, t_pdf, ok = sample_transmittance(med, has_max, max_dist, draw())
        draws += 1
        if strategy == "tr_ex":
            r_sel, r_pos, ux, uy = draw(), draw(), draw(), draw()
            draws += 4
            pos, nrm, flux, surface = fr.emitters.sample(r_sel, r_pos, ux, uy)
    else:
        r_sel, r_pos, ux, uy = draw(), draw(), draw(), draw()
        draws += 4
        pos, nrm, flux, surface = fr.emitters.sample(r_sel, r_pos, ux, uy)
        smp, ok = make_sampler(strategy, has_max, max_dist, o, d, pos, nrm)
        some = ok.copy()
        live = ok | (not may_fail(strategy))                                                 # the samples that go on drawing
        if not live.any():
            zeros["some"] = some
            return out, zeros
        xi = draw()
        draws += np.where(live, 1, 0)
        t_cam, t_pdf = sample_point_normal(smp, xi) if strategy == "pn_ex" else sample_equiangular(smp, has_max, max_dist, xi)
    live = ok | (not may_fail(strategy))
    zeros["some"] = some
    zeros["vertices"] = some.astype(np.int64)
    if is_phase(strategy):
        ux, uy = draw(), draw()
        draws += np.where(live, 2, 0)
    with np.errstate(all="ignore"):
        p = (o + d * _col(t_cam)).astype(np.float32)
        cam_trans = R._div_guarded(med.transmittance(t_cam), t_pdf)
        w_i = (-d).astype(np.float32)
        if is_phase(strategy):
            nd = med.phase_sample(w_i, ux, uy)
            zeros["ext"] = zeros["ext"] + ok.astype(np.int64)
            t2, _, _, mesh2, _ = sc.trace(p, nd)
            for k in np.flatnonzero(ok & (mesh2 >= 0)):
                if int(mesh2[k]) not in fr.light_mesh:
                    continue
                its = sc.trace_full(p[k], nd[k])
                if its is None or R._dot(R._v(its["n_g"]), -nd[k]) < ZERO:
                    continue
                contrib = ((fr.light_mesh[int(mesh2[k])] * med.sigma_s) * ONE).astype(np.float32)
                t_light = R._mag((R._v(its["p"]) - p[k]).astype(np.float32))
                out[k] = ((contrib * cam_trans[k]) * med.transmittance(np.asarray([t_light], np.float32))[0]).astype(np.float32)
            return out, zeros
        d_light = (pos - p).astype(np.float32)
        t_light = R._mag(d_light)
        go = ok & ~((t_light == ZERO) | ~np.isfinite(t_light))
        d_light = (d_light / _col(t_light)).astype(np.float32)
        cos_l = R._dot(nrm, -d_light).astype(np.float32)
        geom = np.where(surface, cos_l / (t_light * t_light), ONE / (t_light * t_light)).astype(np.float32)
        fl = _mul_guarded(flux, geom)
        go &= ~(surface & (cos_l <= ZERO))
        zeros["shadow"] = go.astype(np.int64)
        idx = np.flatnonzero(go)
        if idx.size:
            vis = sc.visible(p[idx], pos[idx]).astype(bool)
            k = idx[vis]
            contrib = ((fl[k] * med.sigma_s[None, :]) * med.phase_eval(w_i[k], d_light[k])).astype(np.float32)
            out[k] = ((contrib * cam_trans[k]) * med.transmittance(t_light[k])).astype(np.float32)
    return out, zeros


# ---- drivers
def block_pixels(sd, b):
    """(px, py) of block b's pixels in compute_mc's order: iy outer, ix inner (mod.rs:420-435)."""
    bx, by, bw, bh = U.block_rect(sd, b)
    c = np.arange(bw * bh)
    return bx + c % bw, by + c // bw


def _finish(sd, spp, px, py, rad, cnt, img, st):
    acc = np.zeros((px.shape[0], 3), np.float32)
    for k in range(spp):                                                                     # im_block.accumulate in sample order
        acc = acc + rad[k::spp]
    img[py, px] = acc * (ONE / F32(spp))                                                     # im_block.scale(1.0 / nb_samples as f32)
    st["camera_samples"] += px.shape[0] * spp
    st["rng_draws"] += int(cnt["draws"].sum())
    st["extension_rays"] += int(cnt["ext"].sum())
    st["shadow_rays"] += int(cnt["shadow"].sum())
    st["vertices"] += int(cnt["vertices"].sum())


class Drivers:
    """The block drivers around one kind of estimator — the plain strategies here (PLAIN below), the MIS families in tests/pnmis_restatement.py.  A kind is its
    evaluate, draws_per_sample, max_draws and check_params; chain(strategy) -> (the strategy whose make_sampler is the None test, the draws a sample takes behind
    the jitter without a sampler, with one), which is all the chain walk knows of a sample; extra_counts, the per-sample flags it reports beside "some", each
    also summed into detail; frame_class; and fixture_key(strategy), under which a fixture's render is cached."""

    def __init__(self, evaluate, draws_per_sample, max_draws, check_params, chain, frame_class, extra_counts=(), fixture_key=lambda strategy: strategy):
        self.evaluate, self.draws_per_sample, self.max_draws, self.check_params, self.chain = evaluate, draws_per_sample, max_draws, check_params, chain
        self.frame_class, self.extra_counts, self.fixture_key = frame_class, tuple(extra_counts), fixture_key
        self.cache = {}

    def _new_detail(self):
        return {"starts": {}, "some": 0, "none": 0, **{k: 0 for k in self.extra_counts}}

    def _add_detail(self, detail, cnt):
        detail["some"] += int(cnt["some"].sum()); detail["none"] += int((~cnt["some"]).sum())
        for k in self.extra_counts:
            detail[k] += int(cnt[k].sum())

    def walk_block(self, fr, b, seed, strategy, spp, use_aa=True, stream_mode=api.STREAM_REFERENCE_ORDER, seed_variant=0):
        """The reference's loop over one block, camera sample after camera sample, draw after draw on orc.Rng: (px, py, radiance [pixels * spp, 3], counts,
        start offsets [pixels] — the draws the block's stream has given when the pixel starts, reference order only)."""
        px, py = block_pixels(fr.sd, b)
        block_rng = orc.Rng(int(seed), seed_variant)
        taken = [0]
        rads, cnts, starts = [], [], []
        for c in range(px.shape[0]):
            starts.append(taken[0])
            pixel_rng = orc.Rng(block_rng.next_u64(), seed_variant) if stream_mode == api.STREAM_PER_SAMPLE else None
            for s in range(spp):
                rng = orc.Rng(pixel_rng.next_u64(), seed_variant) if pixel_rng is not None else block_rng

                def draw():
                    taken[0] += 1
                    return np.asarray([rng.next_f32()], np.float32)

                before = taken[0]
                rad, cnt = self.evaluate(fr, strategy, use_aa, px[c:c + 1], py[c:c + 1], draw)
                assert taken[0] - before == int(cnt["draws"][0]), (strategy, taken[0] - before, cnt["draws"])
                rads.append(rad[0]); cnts.append(cnt)
        counts = {k: np.concatenate([c[k] for c in cnts]) for k in ("draws", "ext", "shadow", "vertices", "some") + self.extra_counts}
        return px, py, np.asarray(rads, np.float32), counts, np.asarray(starts, np.int64)

    def chain_offsets(self, fr, b, seed, strategy, spp, use_aa, seed_variant, s_stream):
        """Where every camera sample of block b starts in the block's stream when the count depends on the data: the walk of the None test alone (the jitter,
        the camera ray's closest hit, the four emitter draws, make_sampler), sample after sample.  [pixels * spp] int64."""
        px, py = block_pixels(fr.sd, b)
        px, py = np.repeat(px, spp), np.repeat(py, spp)
        aa = 2 if use_aa else 0
        decides, without, with_sampler = self.chain(strategy)
        offs, at = np.zeros(px.shape[0], np.int64), 0
        sc = fr.sc
        for i in range(px.shape[0]):
            offs[i] = at
            if use_aa:
                u, v = F32(px[i]) + s_stream[at], F32(py[i]) + s_stream[at + 1]
            else:
                u, v = F32(px[i]) + F32(0.5), F32(py[i]) + F32(0.5)
            o, d = sc.camera_generate(float(u), float(v))
            o, d = o.reshape(1, 3), d.reshape(1, 3)
            t, _, _, mesh, _ = sc.trace(o, d)
            q = s_stream[at + aa:at + aa + 4]
            pos, nrm, _, _ = fr.emitters.sample(q[0:1], q[1:2], q[2:3], q[3:4])
            _, ok = make_sampler(decides, mesh >= 0, t.astype(np.float32), o, d, pos, nrm)
            at += aa + (with_sampler if ok[0] else without)
        return offs, at

    def render(self, fr, seeds, strategy, spp=1, use_aa=True, stream_mode=api.STREAM_REFERENCE_ORDER, seed_variant=0, shard_index=0, shard_count=1):
        """(image HxWx3 f32, the five counters, detail) with every camera sample of a block as one array element.  detail: "starts" {block: [pixels] the draws
        the block's stream has given when each pixel starts} (reference order), "some" / "none": how many samples had / lacked the distance sampler that can
        be None, and the kind's extra counts."""
        self.check_params(strategy, spp, stream_mode, shard_index, shard_count, use_aa)
        sd = fr.sd
        img = np.zeros((sd.height, sd.width, 3), np.float32)
        st = {k: 0 for k in COUNTERS}
        detail = self._new_detail()
        kmax = self.max_draws(strategy, use_aa)
        for b, seed in enumerate(np.asarray(seeds, np.uint64)):
            if b % max(shard_count, 1) != shard_index:
                continue
            px, py = block_pixels(sd, b)
            n_pix = px.shape[0]
            spx, spy = np.repeat(px, spp), np.repeat(py, spp)
            n = n_pix * spp
            if stream_mode == api.STREAM_PER_SAMPLE:
                block_rng = orc.Rng(int(seed), seed_variant)
                table = np.zeros((n, kmax), np.float32)
                for c in range(n_pix):
                    pixel_rng = orc.Rng(block_rng.next_u64(), seed_variant)
                    for s in range(spp):
                        rng = orc.Rng(pixel_rng.next_u64(), seed_variant)
                        table[c * spp + s] = [rng.next_f32() for _ in range(kmax)]
            else:
                s_stream = U.stream(int(seed), seed_variant, n * kmax + kmax)
                dconst = self.draws_per_sample(strategy, use_aa)
                if dconst is not None:
                    offs = np.arange(n, dtype=np.int64) * dconst
                else:
                    offs, _ = self.chain_offsets(fr, b, int(seed), strategy, spp, use_aa, seed_variant, s_stream)
                table = s_stream[offs[:, None] + np.arange(kmax)[None, :]]
                detail["starts"][b] = offs[::spp].copy()
            col = [0]

            def draw():
                col[0] += 1
                return table[:, col[0] - 1].copy()

            rad, cnt = self.evaluate(fr, strategy, use_aa, spx, spy, draw)
            _finish(sd, spp, px, py, rad, cnt, img, st)
            self._add_detail(detail, cnt)
        return img, st, detail

    def render_walk(self, fr, seeds, strategy, spp=1, use_aa=True, stream_mode=api.STREAM_REFERENCE_ORDER, seed_variant=0, shard_index=0, shard_count=1):
        """render through walk_block: (image, counters, detail)."""
        self.check_params(strategy, spp, stream_mode, shard_index, shard_count, use_aa)
        sd = fr.sd
        img = np.zeros((sd.height, sd.width, 3), np.float32)
        st = {k: 0 for k in COUNTERS}
        detail = self._new_detail()
        for b, seed in enumerate(np.asarray(seeds, np.uint64)):
            if b % max(shard_count, 1) != shard_index:
                continue
            px, py, rad, cnt, starts = self.walk_block(fr, b, int(seed), strategy, spp, use_aa, stream_mode, seed_variant)
            _finish(sd, spp, px, py, rad, cnt, img, st)
            if stream_mode == api.STREAM_REFERENCE_ORDER:
                detail["starts"][b] = starts
            self._add_detail(detail, cnt)
        return img, st, detail

    def compute(self, sd, seed=0, strategy="tr_ex", spp=1, use_aa=True, stream_mode=api.STREAM_REFERENCE_ORDER, seed_variant=0):
        """IntegratorPointNormal::compute seed for seed: the block seeds straight from the main sampler seeded as `-r independent:SEED`."""
        fr = self.frame_class(sd)
        seeds = orc.block_seeds(seed, sd.width, sd.height, seed_variant)
        img, st, detail = self.render(fr, seeds, strategy, spp, use_aa, stream_mode, seed_variant)
        return {"seeds": seeds, "image": img, "stats": st, "detail": detail, "frame": fr}

    # the fixtures the CPU and the GPU tests share, each computed once and left unchanged
    def frame(self, name, w=24, h=18):
        if (name, w, h) not in self.cache:
            self.cache[(name, w, h)] = self.frame_class(scene(name, w, h))
        return self.cache[(name, w, h)]

    def fixture(self, name, strategy, spp=3, use_aa=True, stream_mode=api.STREAM_REFERENCE_ORDER, w=24, h=18, seed=7, shard_index=0, shard_count=1):
        """(frame, seeds, image, counters, detail) of one render of scene(name), computed once."""
        key = ("render", name, self.fixture_key(strategy), spp, use_aa, stream_mode, w, h, seed, shard_index, shard_count)
        if key not in self.cache:
            fr = self.frame(name, w, h)
            seeds = orc.block_seeds(seed, w, h)
            self.cache[key] = (fr, seeds) + self.render(fr, seeds, strategy, spp, use_aa, stream_mode, 0, shard_index, shard_count)
        return self.cache[key]


PLAIN = Drivers(evaluate, draws_per_sample, max_draws, check_params, lambda strategy: (strategy, 4, 4 + (3 if is_phase(strategy) else 1)), Frame)
walk_block, chain_offsets, render, render_walk, compute, frame, fixture = (PLAIN.walk_block, PLAIN.chain_offsets, PLAIN.render, PLAIN.render_walk, PLAIN.compute,
                                                                           PLAIN.frame, PLAIN.fixture)


def camera_rays(fr, seeds, strategy, spp, use_aa=True, stream_mode=api.STREAM_REFERENCE_ORDER, seed_variant=0):
    """(px, py, o, d, tfar) of every camera sample of a render, for the quadrature: the jitter alone is evaluated."""
    sd = fr.sd
    out = {k: [] for k in ("px", "py", "o", "d", "has_max", "max_dist")}
    for b, seed in enumerate(np.asarray(seeds, np.uint64)):
        _, _, _, cnt, _ = _rays_of_block(fr, b, int(seed), strategy, spp, use_aa, stream_mode, seed_variant)
        for k in out:
            out[k].append(cnt[k])
    px, py = np.concatenate(out["px"]), np.concatenate(out["py"])
    o, d = np.concatenate(out["o"]), np.concatenate(out["d"])
    tfar = np.where(np.concatenate(out["has_max"]), np.concatenate(out["max_dist"]), F32_MAX).astype(np.float32)
    return px, py, o, d, tfar


def _rays_of_block(fr, b, seed, strategy, spp, use_aa, stream_mode, seed_variant):
    px, py = block_pixels(fr.sd, b)
    spx, spy = np.repeat(px, spp), np.repeat(py, spp)
    n = spx.shape[0]
    if not use_aa:
        u, v = spx.astype(np.float32) + F32(0.5), spy.astype(np.float32) + F32(0.5)
    elif stream_mode == api.STREAM_PER_SAMPLE:
        block_rng = orc.Rng(int(seed), seed_variant)
        j = np.zeros((n, 2), np.float32)
        for c in range(px.shape[0]):
            pixel_rng = orc.Rng(block_rng.next_u64(), seed_variant)
            for s in range(spp):
                rng = orc.Rng(pixel_rng.next_u64(), seed_variant)
                j[c * spp + s] = [rng.next_f32(), rng.next_f32()]
        u, v = spx.astype(np.float32) + j[:, 0], spy.astype(np.float32) + j[:, 1]
    else:
        kmax = max_draws(strategy, use_aa)
        s_stream = U.stream(int(seed), seed_variant, n * kmax + kmax)
        dconst = draws_per_sample(strategy, use_aa)
        offs = np.arange(n, dtype=np.int64) * dconst if dconst is not None else chain_offsets(fr, b, seed, strategy, spp, use_aa, seed_variant, s_stream)[0]
        u, v = spx.astype(np.float32) + s_stream[offs], spy.astype(np.float32) + s_stream[offs + 1]
    rays = [fr.sc.camera_generate(float(a), float(c)) for a, c in zip(u, v)]
    o = np.asarray([r[0] for r in rays], np.float32).reshape(-1, 3)
    d = np.asarray([r[1] for r in rays], np.float32).reshape(-1, 3)
    t, _, _, mesh, _ = fr.sc.trace(o, d)
    return None, None, None, {"px": spx, "py": spy, "o": o, "d": d, "has_max": mesh >= 0, "max_dist": t.astype(np.float32)}, None


# ---- the scenes and fixtures the CPU and the GPU tests share, each computed once and left unchanged
COLOURED = ((0.4, 1.0, 1.5), (1.2, 0.6, 0.1))          # sigma_s, sigma_a: sigma_t = 1.6 in every channel
POINT_LIGHT = {"type": "point", "a": (0.3, 1.5, 0.4), "intensity": (2.0, 1.5, 1.0)}


def floating_light(w, h, tilt_degrees=5.0):
    """One emissive quad of side 1 about (0, 1.8, 0) in the Cornell box's camera and nothing else, its normal (0, cos a, sin a) turned up and a little towards
    the camera: most camera rays miss everything (max_dist = None), the few that reach the quad see its back, and the light's plane passes above the camera,
    so a clamped or point-normal sampler is None for the rays that leave the camera below that plane's direction and Some for the rest."""
    from rustlight_amd import scenes
    a = np.radians(tilt_degrees)
    c, ex, ev, n = np.asarray([0.0, 1.8, 0.0]), np.asarray([1.0, 0.0, 0.0]), np.asarray([0.0, -np.sin(a), np.cos(a)]), [0.0, float(np.cos(a)), float(np.sin(a))]
    corners = [c - 0.5 * ex - 0.5 * ev, c + 0.5 * ex - 0.5 * ev, c + 0.5 * ex + 0.5 * ev, c - 0.5 * ex + 0.5 * ev]
    light = scenes._quad_mesh("Light", np.concatenate(corners).tolist(), n, scenes.matte((0.0, 0.0, 0.0)), emission=(17.0, 12.0, 4.0))
    return scenes.SceneData(w, h, scenes.CBOX_FOV, 1, np.asarray(scenes.CBOX_TO_WORLD, dtype=np.float32), False, [light],
                            scenes.Medium((0.0,) * 3, (1.0,) * 3, scenes.PHASE_ISOTROPIC, 0.0))


def scene(name, w=24, h=18):
    """box: the Cornell box with its grey medium | coloured: a coloured medium with Henyey-Greenstein g = 0.6 | lights: a second area light and a point light
    | floating: floating_light."""
    from rustlight_amd import scenes
    from tests.scene_helpers import add_second_light
    if name == "box":
        return scenes.cbox_medium(w, h, 1.0)
    if name == "coloured":
        return scenes.cbox(w, h, scenes.Medium(COLOURED[1], COLOURED[0], scenes.PHASE_HG, 0.6))
    if name == "lights":
        sd = add_second_light(scenes.cbox_medium(w, h, 1.0))
        sd.lights.append(dict(POINT_LIGHT))
        return sd
    if name == "floating":
        return floating_light(w, h)
    raise KeyError(name)
