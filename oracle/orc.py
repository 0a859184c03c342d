"""ctypes binding of the CPU oracle (TEST INFRASTRUCTURE — see oracle/rl_oracle.cpp).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from rustlight_amd import abi
from rustlight_amd import scenes as S
from rustlight_amd.api import VPL_ALL, VPL_SURFACE, VPL_VOLUME, VPL_WORDS     # rl_vpl_option, RL_VPL_WORDS: defined once, beside the product's binding

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "librl_oracle.so")
VPL_MAX_PATHS = 1 << 18           # RL_VPL_MAX_PATHS: orc_vpl_generate gives up after as many light paths
VPL_DEPTH_CAP = 2048              # ORC_DEPTH_CAP, the product's kDepthCap: no light path has more vertices


class OrcPathParams(C.Structure):
    _fields_ = [("spp", C.c_uint32), ("has_min_depth", C.c_int32), ("min_depth", C.c_uint32),
                ("has_max_depth", C.c_int32), ("max_depth", C.c_uint32), ("has_rr_depth", C.c_int32),
                ("rr_depth", C.c_uint32), ("strategy", C.c_int32), ("single_scattering", C.c_int32),
                ("stream_mode", C.c_int32), ("seed_variant", C.c_int32), ("shard_index", C.c_uint32),
                ("shard_count", C.c_uint32), ("eval_order", C.c_int32)]


class OrcMcParams(C.Structure):
    _fields_ = [("spp", C.c_uint32), ("stream_mode", C.c_int32), ("seed_variant", C.c_int32), ("shard_index", C.c_uint32),
                ("shard_count", C.c_uint32), ("has_max_distance", C.c_int32), ("max_distance", C.c_float),
                ("normal_correction", C.c_int32), ("nb_bsdf_samples", C.c_uint32), ("nb_light_samples", C.c_uint32)]


class OrcStats(C.Structure):
    _fields_ = [("camera_samples", C.c_uint64), ("vertices", C.c_uint64), ("extension_rays", C.c_uint64),
                ("shadow_rays", C.c_uint64), ("rng_draws", C.c_uint64), ("threads", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class OrcLightStats(C.Structure):
    _fields_ = [("splats", C.c_uint64), ("splats_invalid", C.c_uint64), ("splats_saturated", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def build(force: bool = False) -> str:
    srcs = [os.path.join(_HERE, f) for f in ("rl_oracle.cpp", "rl_oracle.h", "detmath.h")]
    srcs.append(os.path.join(_HERE, "..", "include", "rustlight_amd.h"))
    stale = force or not os.path.exists(_LIB_PATH) or not os.path.exists(os.path.join(_HERE, "librl_oracle_timing.so")) or any(
        os.path.exists(s) and os.path.getmtime(s) > os.path.getmtime(_LIB_PATH) for s in srcs)
    if stale:
        subprocess.check_call(["make", "-C", _HERE, "-s", "-B"])
    return _LIB_PATH


_lib = None
_timing = False


def use_timing_build(on: bool = True):
    """bench.py's cpu_baseline: load librl_oracle_timing.so (-O3, libm transcendentals, FMA allowed) instead of the parity build.
    Must be called before the first use of the module; the timing build is never used as a checker."""
    global _timing
    assert _lib is None, "oracle already loaded"
    _timing = on


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(os.path.join(_HERE, "librl_oracle_timing.so") if _timing else _LIB_PATH)
        L.orc_scene_create.restype = C.c_void_p
        L.orc_scene_destroy.argtypes = [C.c_void_p]
        L.orc_scene_set_camera.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_int,
                                           C.POINTER(C.c_float), C.c_int]
        L.orc_scene_add_bitmap.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
        L.orc_scene_add_mesh.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_uint32),
                                         C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                         C.POINTER(abi.BsdfDesc), C.POINTER(C.c_float)]
        L.orc_scene_set_medium.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_float]
        L.orc_scene_set_mesh_emission.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int]
        L.orc_scene_build.argtypes = [C.c_void_p]
        L.orc_scene_add_point_light.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.orc_scene_add_directional_light.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.orc_scene_set_environment.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.orc_scene_set_ats.argtypes = [C.c_void_p, C.c_int]
        L.orc_ats_probe.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.orc_ats_dump.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.orc_env_probe.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.orc_scene_set_environment_map.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
        L.orc_rng_seed.argtypes = [C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
        L.orc_rng_next_u64.argtypes = [C.POINTER(C.c_uint64)]
        L.orc_rng_next_u64.restype = C.c_uint64
        L.orc_rng_next_f32.argtypes = [C.POINTER(C.c_uint64)]
        L.orc_rng_next_f32.restype = C.c_float
        L.orc_block_count.argtypes = [C.c_uint32, C.c_uint32]
        L.orc_block_count.restype = C.c_size_t
        L.orc_generate_block_seeds.argtypes = [C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
        L.orc_math_batch.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.orc_camera_generate.argtypes = [C.c_void_p, C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.orc_camera_sample_direct.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.orc_scene_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
        L.orc_bvh_dump.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                   C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.orc_trace_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int,
                                      C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                      C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.orc_visible_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint8)]
        L.orc_trace_full.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.orc_bsdf_probe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.orc_sample_light.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_float)]
        L.orc_compute_pixel.argtypes = [C.c_void_p, C.POINTER(OrcPathParams), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64),
                                        C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.orc_compute_pixel.restype = C.c_uint64
        L.orc_render_path.argtypes = [C.c_void_p, C.POINTER(OrcPathParams), C.POINTER(C.c_uint64), C.c_size_t,
                                      C.POINTER(C.c_float), C.c_int, C.POINTER(OrcStats)]
        L.orc_render_mc.argtypes = [C.c_void_p, C.c_int, C.POINTER(OrcMcParams), C.POINTER(C.c_uint64), C.c_size_t,
                                    C.POINTER(C.c_float), C.c_int, C.POINTER(OrcStats)]
        L.orc_render_light.argtypes = [C.c_void_p, C.POINTER(OrcPathParams), C.POINTER(C.c_uint64), C.c_size_t,
                                       C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_int, C.POINTER(OrcStats),
                                       C.POINTER(OrcLightStats)]
        L.orc_vpl_generate.restype = C.c_long
        L.orc_vpl_generate.argtypes = [C.c_void_p, C.POINTER(OrcPathParams), C.c_uint32, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_size_t,
                                       C.POINTER(C.c_uint64)]
        L.orc_render_vpl.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_uint64), C.c_size_t, C.c_uint32,
                                     C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
        L.orc_stratified_draws.argtypes = [C.c_size_t, C.POINTER(C.c_uint64), C.c_uint32, C.c_int, C.c_size_t, C.POINTER(C.c_int32),
                                           C.POINTER(C.c_float)]
        _lib = L
    return _lib


def path_params(spp=1, min_depth=0, max_depth=None, rr_depth=0, strategy=0, single_scattering=False,
                stream_mode=1, seed_variant=0, shard_index=0, shard_count=1, eval_order=0) -> OrcPathParams:
    p = OrcPathParams()
    p.spp = spp
    p.has_min_depth, p.min_depth = (0, 0) if min_depth is None else (1, min_depth)
    p.has_max_depth, p.max_depth = (0, 0) if max_depth is None else (1, max_depth)
    p.has_rr_depth, p.rr_depth = (0, 0) if rr_depth is None else (1, rr_depth)
    p.strategy = strategy
    p.single_scattering = int(single_scattering)
    p.stream_mode = stream_mode
    p.seed_variant = seed_variant
    p.shard_index, p.shard_count = shard_index, shard_count
    p.eval_order = eval_order
    return p


class Rng:
    def __init__(self, seed: int, variant: int = 0):
        self.state = (C.c_uint64 * 4)()
        lib().orc_rng_seed(seed, variant, self.state)

    @classmethod
    def from_state(cls, s):
        r = cls.__new__(cls)
        r.state = (C.c_uint64 * 4)(*s)
        return r

    def next_u64(self) -> int:
        return int(lib().orc_rng_next_u64(self.state))

    def next_f32(self) -> float:
        return float(lib().orc_rng_next_f32(self.state))


def stratified_draws(pixel_seeds, spp: int, pattern, seed_variant: int = 0) -> np.ndarray:
    """The oracle's RL_STREAM_STRATIFIED sampler with the contract of api.stratified_draws: pixel p, whose per-sample-mode seed is pixel_seeds[p],
    walks its spp samples; each sample makes the calls of `pattern` (1 = next(), 2 = next2d()).  float32 [n_pixels, spp, sum(pattern)]."""
    seeds = np.ascontiguousarray(pixel_seeds, dtype=np.uint64).reshape(-1)
    pat = np.ascontiguousarray(pattern, dtype=np.int32).reshape(-1)
    out = np.zeros((seeds.shape[0], spp, int(pat.sum())), dtype=np.float32)
    rc = lib().orc_stratified_draws(seeds.shape[0], abi.u64ptr(seeds), spp, seed_variant, pat.shape[0], pat.ctypes.data_as(C.POINTER(C.c_int32)),
                                    abi.fptr(out))
    if rc != 0:
        raise RuntimeError(f"orc_stratified_draws failed: {rc}")
    return out


def block_seeds(master_seed: int, width: int, height: int, variant: int = 0) -> np.ndarray:
    """`-r independent:SEED` then generate_img_blocks: one next_u64 per block, x-major."""
    r = Rng(master_seed, variant)
    n = lib().orc_block_count(width, height)
    seeds = np.zeros(n, dtype=np.uint64)
    lib().orc_generate_block_seeds(r.state, width, height, abi.u64ptr(seeds))
    return seeds


class Scene:
    def __init__(self, sd: S.SceneData):
        L = lib()
        self.sd = sd
        self.h = C.c_void_p(L.orc_scene_create())
        tw = np.ascontiguousarray(sd.to_world, dtype=np.float32)
        rc = L.orc_scene_set_camera(self.h, sd.width, sd.height, sd.fov, sd.fov_axis, abi.fptr(tw), int(sd.flip))
        assert rc == 0
        for (w, h, rgb) in sd.bitmaps:
            a = np.ascontiguousarray(rgb, dtype=np.float32)
            L.orc_scene_add_bitmap(self.h, w, h, abi.fptr(a))
        for m in sd.meshes:
            v, i, n, uv, e = abi.mesh_arrays(m)
            bd = abi.bsdf_desc(m.bsdf)
            rc = L.orc_scene_add_mesh(self.h, abi.fptr(v), v.shape[0], abi.u32ptr(i), i.shape[0], abi.fptr(n),
                                      abi.fptr(uv), C.byref(bd), abi.fptr(e))
            assert rc >= 0
            if getattr(m, "emission_kind", None):          # EmissionType::HSV / Texture (geometry.rs:99-104)
                ek = m.emission_kind
                assert L.orc_scene_set_mesh_emission(self.h, rc, 1 if ek[0] == "hsv" else 2, float(ek[1]), int(ek[2]) if len(ek) > 2 else -1) == 0
        if sd.medium is not None:
            sa = np.asarray(sd.medium.sigma_a, dtype=np.float32)
            ss = np.asarray(sd.medium.sigma_s, dtype=np.float32)
            L.orc_scene_set_medium(self.h, abi.fptr(sa), abi.fptr(ss), sd.medium.phase, sd.medium.g)
        for lt in sd.lights:
            a = np.asarray(lt["a"], np.float32); b = np.asarray(lt["intensity"], np.float32)
            (L.orc_scene_add_point_light if lt["type"] == "point" else L.orc_scene_add_directional_light)(self.h, abi.fptr(a), abi.fptr(b))
        if sd.environment is not None:
            e = np.asarray(sd.environment, np.float32)
            L.orc_scene_set_environment(self.h, abi.fptr(e))
        if sd.environment_map is not None:
            em = np.ascontiguousarray(sd.environment_map, np.float32)
            L.orc_scene_set_environment_map(self.h, em.shape[1], em.shape[0], abi.fptr(em))
        L.orc_scene_set_ats(self.h, int(getattr(sd, "use_ats", False)))
        L.orc_scene_build(self.h)

    def ats_dump(self):
        """(nodes [n, 16] f32 with the 4 link words as int32 bit patterns, light_emitter, light_prim) of the light tree."""
        nn, nl = C.c_uint64(), C.c_uint64()
        lib().orc_ats_dump(self.h, C.byref(nn), None, C.byref(nl), None, None)
        nodes = np.zeros((nn.value, 16), np.float32); le = np.zeros(nl.value, np.int32); lp = np.zeros(nl.value, np.int32)
        lib().orc_ats_dump(self.h, C.byref(nn), abi.fptr(nodes), C.byref(nl), le.ctypes.data_as(C.POINTER(C.c_int32)), lp.ctypes.data_as(C.POINTER(C.c_int32)))
        return nodes, le, lp

    def ats_probe(self, kind, values):
        a = np.asarray(values, np.float32); out = np.zeros(4, np.float32)
        assert lib().orc_ats_probe(self.h, kind, abi.fptr(a), abi.fptr(out)) == 0
        return out

    def env_probe(self, kind, values):
        a = np.asarray(values, np.float32); out = np.zeros(8, np.float32)
        assert lib().orc_env_probe(self.h, kind, abi.fptr(a), abi.fptr(out)) == 0
        return out

    def __del__(self):
        try:
            lib().orc_scene_destroy(self.h)
        except Exception:
            pass

    def info(self):
        nn, npr, ne = C.c_uint64(), C.c_uint64(), C.c_uint64()
        bs = (C.c_float * 4)()
        lib().orc_scene_info(self.h, C.byref(nn), C.byref(npr), C.byref(ne), bs)
        return {"nodes": nn.value, "prims": npr.value, "emitters": ne.value, "bsphere": list(bs)}

    def bvh(self):
        inf = self.info()
        boxes = np.zeros((inf["nodes"], 6), dtype=np.float32)
        info = np.zeros(inf["nodes"], dtype=np.uint64)
        count = np.zeros(inf["nodes"], dtype=np.uint64)
        pm = np.zeros(inf["prims"], dtype=np.int32)
        pt = np.zeros(inf["prims"], dtype=np.int32)
        lib().orc_bvh_dump(self.h, abi.fptr(boxes), abi.u64ptr(info), abi.u64ptr(count),
                           pm.ctypes.data_as(C.POINTER(C.c_int32)), pt.ctypes.data_as(C.POINTER(C.c_int32)))
        return boxes, info, count, pm, pt

    def camera_generate(self, px, py):
        o = (C.c_float * 3)()
        d = (C.c_float * 3)()
        lib().orc_camera_generate(self.h, px, py, o, d)
        return np.array(o[:], dtype=np.float32), np.array(d[:], dtype=np.float32)

    def sample_direct(self, p):
        """Camera::sample_direct (camera.rs:94-118): None, or (importance, screen position in pixels)."""
        pp = np.asarray(p, np.float32); out = np.zeros(3, np.float32)
        if not lib().orc_camera_sample_direct(self.h, abi.fptr(pp), abi.fptr(out)):
            return None
        return float(out[0]), out[1:3]

    def trace(self, origins, directions, brute=False):
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        n = o.shape[0]
        t = np.zeros(n, np.float32); u = np.zeros(n, np.float32); v = np.zeros(n, np.float32)
        m = np.zeros(n, np.int32); tr = np.zeros(n, np.int32)
        lib().orc_trace_batch(self.h, n, abi.fptr(o), abi.fptr(d), int(brute), abi.fptr(t), abi.fptr(u), abi.fptr(v),
                              m.ctypes.data_as(C.POINTER(C.c_int32)), tr.ctypes.data_as(C.POINTER(C.c_int32)))
        return t, u, v, m, tr

    def visible(self, p0, p1):
        a = np.ascontiguousarray(p0, dtype=np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(p1, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(a.shape[0], np.uint8)
        lib().orc_visible_batch(self.h, a.shape[0], abi.fptr(a), abi.fptr(b), out.ctypes.data_as(C.POINTER(C.c_uint8)))
        return out

    def trace_full(self, o, d):
        oo = np.asarray(o, dtype=np.float32); dd = np.asarray(d, dtype=np.float32)
        out = np.zeros(17, np.float32)
        hit = lib().orc_trace_full(self.h, abi.fptr(oo), abi.fptr(dd), abi.fptr(out))
        if not hit:
            return None
        return {"t": out[0], "p": out[1:4], "n_g": out[4:7], "n_s": out[7:10], "uv": out[10:12], "wi": out[12:15],
                "mesh": int(out[15]), "tri": int(out[16])}

    def bsdf_sample(self, mesh, wi, s):
        w = np.asarray(wi, np.float32); ss = np.asarray(s, np.float32); out = np.zeros(9, np.float32)
        lib().orc_bsdf_probe(self.h, mesh, 0, abi.fptr(w), abi.fptr(ss), abi.fptr(out))
        if out[0] == 0:
            return None
        return {"weight": out[1:4], "d": out[4:7], "pdf": out[7], "pdf_kind": int(out[8])}

    def bsdf_eval(self, mesh, wi, wo):
        w = np.asarray(wi, np.float32); o = np.asarray(wo, np.float32); out = np.zeros(3, np.float32)
        lib().orc_bsdf_probe(self.h, mesh, 1, abi.fptr(w), abi.fptr(o), abi.fptr(out))
        return out

    def bsdf_pdf(self, mesh, wi, wo):
        w = np.asarray(wi, np.float32); o = np.asarray(wo, np.float32); out = np.zeros(2, np.float32)
        lib().orc_bsdf_probe(self.h, mesh, 2, abi.fptr(w), abi.fptr(o), abi.fptr(out))
        return float(out[0])

    def sample_light(self, p, r_sel, r, ux, uy):
        pp = np.asarray(p, np.float32); out = np.zeros(15, np.float32)
        lib().orc_sample_light(self.h, abi.fptr(pp), r_sel, r, ux, uy, abi.fptr(out))
        return {"pdf": out[0], "p": out[1:4], "n": out[4:7], "d": out[7:10], "weight": out[10:13], "emitter": int(out[13]), "pdf_kind": int(out[14])}

    def compute_pixel(self, ix, iy, rng: Rng, **kw):
        p = path_params(**kw)
        rgb = (C.c_float * 3)(); nv = C.c_uint64(); ns = C.c_uint64()
        draws = lib().orc_compute_pixel(self.h, C.byref(p), ix, iy, rng.state, rgb, C.byref(nv), C.byref(ns))
        return np.array(rgb[:], np.float32), int(draws), nv.value, ns.value

    def render(self, master_seed=0, threads=0, seeds=None, **kw):
        p = path_params(**kw)
        sd = self.sd
        if seeds is None:
            seeds = block_seeds(master_seed, sd.width, sd.height, p.seed_variant)
        img = np.zeros((sd.height, sd.width, 3), dtype=np.float32)
        st = OrcStats()
        rc = lib().orc_render_path(self.h, C.byref(p), abi.u64ptr(seeds), seeds.shape[0], abi.fptr(img), threads, C.byref(st))
        if rc != 0:
            raise RuntimeError(f"orc_render_path failed: {rc}")
        return img, st.as_dict()


def _render_mc(self, kind, master_seed=0, threads=0, seeds=None, spp=1, stream_mode=1, seed_variant=0, shard_index=0, shard_count=1,
               max_distance=1.0, normal_correction=False, nb_bsdf_samples=1, nb_light_samples=1):
    """ao (kind 0: IntegratorAO) / direct (kind 1: IntegratorDirect) through compute_mc."""
    p = OrcMcParams()
    p.spp, p.stream_mode, p.seed_variant, p.shard_index, p.shard_count = spp, stream_mode, seed_variant, shard_index, shard_count
    p.has_max_distance, p.max_distance = (0, 0.0) if max_distance is None else (1, max_distance)
    p.normal_correction = int(normal_correction)
    p.nb_bsdf_samples, p.nb_light_samples = nb_bsdf_samples, nb_light_samples
    sd = self.sd
    if seeds is None:
        seeds = block_seeds(master_seed, sd.width, sd.height, seed_variant)
    img = np.zeros((sd.height, sd.width, 3), dtype=np.float32)
    st = OrcStats()
    rc = lib().orc_render_mc(self.h, kind, C.byref(p), abi.u64ptr(seeds), seeds.shape[0], abi.fptr(img), threads, C.byref(st))
    if rc != 0:
        raise RuntimeError(f"orc_render_mc failed: {rc}")
    return img, st.as_dict()


def _render_light(self, seeds=None, spp=1, min_depth=0, max_depth=None, rr_depth=0, strategy=0, seed_variant=0, stream_mode=1, master_seed=0,
                  threads=0, want_f64=False):
    """IntegratorLightTracing as rl_render_light computes it (the keyword arguments of api.Context.render_light; strategy: 0 = all, 1 = surface,
    2 = volume): (image HxWx3 f32, stats dict) or, with want_f64, (image, stats, f64 HxWx3: every pixel's clamped splats summed without
    quantisation, times 1 / spp, counts HxW: the splats every pixel took).  stats carry splats / splats_invalid / splats_saturated as the GPU's."""
    p = path_params(spp=spp, min_depth=min_depth, max_depth=max_depth, rr_depth=rr_depth, strategy=strategy, stream_mode=stream_mode,
                    seed_variant=seed_variant)
    sd = self.sd
    if seeds is None:
        seeds = block_seeds(master_seed, sd.width, sd.height, seed_variant)
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    img = np.zeros((sd.height, sd.width, 3), dtype=np.float32)
    f64 = np.zeros((sd.height, sd.width, 3), dtype=np.float64) if want_f64 else None
    cnt = np.zeros((sd.height, sd.width), dtype=np.uint32) if want_f64 else None
    st, lst = OrcStats(), OrcLightStats()
    rc = lib().orc_render_light(self.h, C.byref(p), abi.u64ptr(seeds), seeds.shape[0], abi.fptr(img),
                                f64.ctypes.data_as(C.POINTER(C.c_double)) if want_f64 else None,
                                cnt.ctypes.data_as(C.POINTER(C.c_uint32)) if want_f64 else None, threads, C.byref(st), C.byref(lst))
    if rc != 0:
        raise RuntimeError(f"orc_render_light failed: {rc}")
    d = dict(st.as_dict(), **lst.as_dict())
    return (img, d, f64, cnt) if want_f64 else (img, d)


def _no_environment(sd):
    # vpl refuses environment emitters; the checker must fail loudly on one rather than give an image
    assert sd.environment is None and sd.environment_map is None, "vpl: environment emitters are refused"


def _vpl_generate(self, state, nb_vpl=128, max_depth=None, rr_depth=0, option_vpl=VPL_ALL):
    """(records [n, 24] u32, paths shot, sampler state after, {camera_samples, vertices, extension_rays, rng_draws}) as rl_vpl_generate."""
    _no_environment(self.sd)
    p = path_params(max_depth=max_depth, rr_depth=rr_depth)
    st = np.array(state, dtype=np.uint64).copy()
    cap = nb_vpl + VPL_DEPTH_CAP + 1                # the host's nb_vpl + kDepthCap + 1: the last path adds at most one VPL per vertex
    words = np.zeros(cap * VPL_WORDS, np.uint32)
    counts = np.zeros(5, np.uint64)
    n = lib().orc_vpl_generate(self.h, C.byref(p), nb_vpl, option_vpl, abi.u64ptr(st), abi.u32ptr(words), cap, abi.u64ptr(counts))
    assert n >= 0, "generation did not end"
    stats = {"camera_samples": int(counts[1]), "vertices": int(counts[2]), "extension_rays": int(counts[3]), "rng_draws": int(counts[4])}
    return words[: n * VPL_WORDS].reshape(n, VPL_WORDS), int(counts[1]), st, stats


def _render_vpl(self, records, n_paths, seeds, spp=1, option_lt=VPL_ALL, seed_variant=0, shard_index=0, shard_count=1, literal_miss=False):
    """(image HxWx3 f32, {camera_samples, extension_rays, shadow_rays, rng_draws, gather_surface, gather_volume}) as rl_render_vpl."""
    _no_environment(self.sd)
    rec = np.ascontiguousarray(records, dtype=np.uint32)
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    img = np.zeros((self.sd.height, self.sd.width, 3), np.float32)
    counts = np.zeros(6, np.uint64)
    rc = lib().orc_render_vpl(self.h, abi.u32ptr(rec), rec.shape[0], n_paths, option_lt, abi.u64ptr(seeds), seeds.shape[0], spp, seed_variant,
                              shard_index, shard_count, int(literal_miss), abi.fptr(img), abi.u64ptr(counts))
    if rc != 0:
        raise RuntimeError(f"orc_render_vpl failed: {rc}")
    keys = ("camera_samples", "extension_rays", "shadow_rays", "rng_draws", "gather_surface", "gather_volume")
    return img, {k: int(v) for k, v in zip(keys, counts)}


def vpl_compute(sd, seed=0, nb_vpl=128, spp=1, max_depth=None, rr_depth=0, option_vpl=VPL_ALL, option_lt=VPL_ALL, seed_variant=0, literal_miss=False):
    """IntegratorVPL::compute seed for seed: the main sampler seeded as `-r independent:SEED`, generation, block seeds from the advanced sampler, gather."""
    sc = Scene(sd)
    rng = Rng(seed, seed_variant)
    rec, n_paths, after, gstats = sc.vpl_generate(rng.state, nb_vpl, max_depth, rr_depth, option_vpl)      # after: the sampler as the generation leaves it
    st = after.copy()
    seeds = np.zeros(lib().orc_block_count(sd.width, sd.height), np.uint64)
    lib().orc_generate_block_seeds(abi.u64ptr(st), sd.width, sd.height, abi.u64ptr(seeds))
    img, rstats = sc.render_vpl(rec, n_paths, seeds, spp, option_lt, seed_variant, literal_miss=literal_miss)
    return {"records": rec, "n_paths": n_paths, "state": after, "gen_stats": gstats, "seeds": seeds, "image": img, "stats": rstats}


Scene.render_light = _render_light
Scene.vpl_generate = _vpl_generate
Scene.render_vpl = _render_vpl
Scene.render_ao = lambda self, **kw: _render_mc(self, 0, **kw)
Scene.render_direct = lambda self, **kw: _render_mc(self, 1, **kw)
