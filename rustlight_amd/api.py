"""ctypes binding of the product C-ABI (include/rustlight_amd.h) + the Python mirror of rustlight's
`Integrator` surface for the `path` hot path.

The library must already be built in-tree (``python -m rustlight_amd.build`` or
``__graft_entry__.build()``); there is no CPU fallback — on a machine without a GPU
``Context`` raises ``NoDeviceError`` (RL_ERR_NO_DEVICE).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import time
from typing import Optional

import numpy as np

from . import abi
from . import scenes as S

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librustlight_amd.so")

RL_OK = 0
RL_ERR_NO_DEVICE = -2
STRATEGY_ALL, STRATEGY_BSDF, STRATEGY_EMITTER = 0, 1, 2
STREAM_REFERENCE_ORDER, STREAM_PER_SAMPLE, STREAM_STRATIFIED = 0, 1, 2      # rl_stream_mode; STRATIFIED: rustlight's StratifiedSampler (`-r stratified`)
PIPELINE_AUTO, PIPELINE_WAVEFRONT, PIPELINE_FUSED = 0, 1, 2
NUMERICS_EXACT, NUMERICS_FAST = 0, 1
LIGHT_ALL, LIGHT_SURFACE, LIGHT_VOLUME = 0, 1, 2          # rl_light_strategy: `light-tracing -s all|surface|volume`
VPL_ALL, VPL_SURFACE, VPL_VOLUME = 0, 1, 2                # rl_vpl_option: `vpl -v / -l all|surface|volume`
LIGHT_STREAMS = ("reference", "per_path")                 # how the light paths of vpl / vol-primitivies draw: rl_vpl_generate | rl_vpl_generate_paths
VPL_WORDS = 24                                            # RL_VPL_WORDS: u32 per VPL record (rl_vpl_read)
TREE_BUILDS = ("host", "device")                          # where the photon tree of vol-primitivies is built: rl_photon_map_build | rl_photon_map_build_device
PHOTON_TREE_GROUP_PHOTONS = 2048                          # RL_PHOTON_TREE_GROUP_PHOTONS: photons one workgroup of the device build finishes in LDS
PHOTON_RADIUS_DEFAULT = 0.001                             # RL_PHOTON_RADIUS_DEFAULT: the radius the reference hard-codes (vol_primitives.rs:618)
BEAM_WORDS = 12                                           # RL_BEAM_WORDS: u32 per beam record (rl_beam_read)
BEAM_MAX = 1 << 17                                        # RL_BEAM_MAX: the most beams a beam pass is asked for
PLANE_FORMS = ("serial", "lanes")                         # how the plane pass of plane-single runs: rl_plane_generate | rl_plane_generate_lanes
PLANE_TREE_GROUP_PLANES = 1024                            # RL_PLANE_TREE_GROUP_PLANES: planes one workgroup of the device build finishes in LDS
PLANE_WORDS = 18                                          # RL_PLANE_WORDS: u32 per plane record (rl_plane_read)
PLANE_UV, PLANE_VT, PLANE_UT, PLANE_UALPHAT = 0, 1, 2, 3  # rl_plane_type
PLANE_STRATEGIES = ("uv", "vt", "ut", "average", "discrete_mis", "ualpha", "cmis")      # rl_plane_strategy, by value: `plane-single -s`
PN_STRATEGIES = ("tr_ex", "tr_phase", "eq_ex", "eq_phase", "eq_clamped_ex", "eq_clamped_phase", "pn_ex")      # rl_pn_strategy, by value: `point-normal -s`
# rl_pn_taylor_strategy, by value: `point-normal-taylor -s`
PN_TAYLOR_STRATEGIES = ("eq_phase_taylor_ex", "eq_tr_taylor_ex", "eq_clamped_phase_taylor_ex", "eq_clamped_tr_taylor_ex", "pn_tr_taylor_ex", "pn_phase_taylor_ex")
# `point-normal-ats -s`: the plain names (rl_pn_ats_family 0) and the Taylor names (1), each with its family's strategy value
PN_ATS_STRATEGIES = PN_STRATEGIES + PN_TAYLOR_STRATEGIES
RL_ERR_UNSUPPORTED, RL_ERR_NO_EMITTER = -7, -8

# every symbol include/rustlight_amd.h declares (tests check the .so exports all of them)
PUBLIC_SYMBOLS = [
    "rl_scene_create", "rl_scene_create_from_desc", "rl_scene_destroy", "rl_scene_set_camera", "rl_scene_set_camera_matrices", "rl_scene_get_camera_matrices", "rl_scene_set_mesh_emission", "rl_scene_override_light_emission", "rl_scene_scale_image", "rl_scene_add_mesh",
    "rl_scene_add_bitmap", "rl_scene_set_medium", "rl_scene_add_point_light", "rl_scene_add_directional_light",
    "rl_scene_set_environment", "rl_scene_set_environment_map", "rl_scene_build_emitters", "rl_scene_enable_ats", "rl_scene_load_pbrt", "rl_scene_load_mitsuba", "rl_scene_load",
    "rl_scene_image_size", "rl_scene_counts", "rl_sampler_seed", "rl_sampler_next_u64", "rl_sampler_next_f32",
    "rl_path_params_default", "rl_device_count", "rl_context_create", "rl_context_destroy", "rl_context_set_option", "rl_context_get_option", "rl_last_error", "rl_block_count",
    "rl_generate_block_seeds", "rl_render_path", "rl_render_path_frames", "rl_multi_create", "rl_multi_destroy", "rl_multi_info", "rl_multi_describe", "rl_multi_shard_stats", "rl_multi_render_path", "rl_render_ao", "rl_render_direct", "rl_render_light", "rl_vpl_generate", "rl_vpl_generate_paths", "rl_vpl_info", "rl_vpl_read", "rl_vpl_destroy", "rl_render_vpl", "rl_photon_map_build", "rl_photon_map_info", "rl_photon_map_destroy", "rl_render_bre", "rl_photon_tree_build", "rl_photon_map_build_device", "rl_photon_tree_build_device", "rl_photon_map_read", "rl_beam_generate", "rl_beam_generate_paths", "rl_beam_info", "rl_beam_read", "rl_beam_destroy", "rl_beam_split", "rl_beam_tree_build", "rl_beam_map_build", "rl_beam_map_build_words", "rl_beam_map_info", "rl_beam_map_read", "rl_beam_map_destroy", "rl_render_beams", "rl_pplane_generate", "rl_pplane_generate_paths", "rl_pplane_info", "rl_pplane_read", "rl_pplane_destroy", "rl_pplane_map_build", "rl_pplane_map_build_words", "rl_pplane_map_info", "rl_pplane_map_read", "rl_pplane_map_destroy", "rl_render_photon_planes", "rl_vrl_map_build", "rl_vrl_map_build_words", "rl_vrl_map_info", "rl_vrl_map_read", "rl_vrl_map_destroy", "rl_render_vrl", "rl_plane_generate", "rl_plane_info", "rl_plane_read", "rl_plane_destroy", "rl_plane_tree_build", "rl_plane_map_build", "rl_plane_map_info", "rl_plane_map_read", "rl_plane_map_destroy", "rl_plane_generate_lanes", "rl_plane_map_build_device", "rl_plane_tree_build_device", "rl_render_plane_single", "rl_render_plane_uncorrelated", "rl_point_normal_params_default", "rl_render_point_normal", "rl_point_normal_mis_params_default", "rl_render_point_normal_mis", "rl_point_normal_taylor_params_default", "rl_render_point_normal_taylor", "rl_point_normal_ats_params_default", "rl_render_point_normal_ats", "rl_trace_batch", "rl_visible_batch", "rl_load_pfm", "rl_load_image", "rl_save_pfm", "rl_save_png", "rl_save_exr", "rl_save_image", "rl_build_info",
]


class PointNormalParams(C.Structure):
    """rl_point_normal_params (include/rustlight_amd.h): IntegratorPointNormal's fields that are built, and how the call runs."""
    _fields_ = [("spp", C.c_uint32), ("strategy", C.c_int32), ("use_aa", C.c_int32), ("stream_mode", C.c_int32), ("seed_variant", C.c_int32),
                ("shard_index", C.c_uint32), ("shard_count", C.c_uint32)]


class PointNormalMisParams(C.Structure):
    """rl_point_normal_mis_params (include/rustlight_amd.h): rl_point_normal_params' fields for IntegratorPointNormal with use_mis."""
    _fields_ = [("spp", C.c_uint32), ("strategy", C.c_int32), ("use_aa", C.c_int32), ("stream_mode", C.c_int32), ("seed_variant", C.c_int32),
                ("shard_index", C.c_uint32), ("shard_count", C.c_uint32)]


class PointNormalTaylorParams(C.Structure):
    """rl_point_normal_taylor_params (include/rustlight_amd.h): rl_point_normal_params' fields for IntegratorPointNormal's Taylor strategies."""
    _fields_ = [("spp", C.c_uint32), ("strategy", C.c_int32), ("use_aa", C.c_int32), ("stream_mode", C.c_int32), ("seed_variant", C.c_int32),
                ("shard_index", C.c_uint32), ("shard_count", C.c_uint32)]


class PointNormalAtsParams(C.Structure):
    """rl_point_normal_ats_params (include/rustlight_amd.h): rl_point_normal_params' fields, then the name family, for IntegratorPointNormal over the light tree."""
    _fields_ = [("spp", C.c_uint32), ("strategy", C.c_int32), ("use_aa", C.c_int32), ("stream_mode", C.c_int32), ("seed_variant", C.c_int32),
                ("shard_index", C.c_uint32), ("shard_count", C.c_uint32), ("family", C.c_int32)]


class RustlightError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__(f"rustlight_amd error {code}: {msg}")
        self.code = code


class NoDeviceError(RustlightError):
    pass


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -m rustlight_amd.build` "
                           "(the HIP extension is mandatory, there is no fallback path)")
    L = C.CDLL(LIB_PATH)
    vp, f32p, u32p, u64p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    L.rl_context_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.rl_context_get_option.argtypes = [vp, C.c_char_p]
    L.rl_context_get_option.restype = C.c_char_p
    L.rl_scene_create.argtypes = [C.POINTER(vp)]
    L.rl_scene_create_from_desc.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(vp)]
    L.rl_scene_destroy.argtypes = [vp]
    L.rl_scene_destroy.restype = None
    L.rl_scene_set_camera.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_float, C.c_int, f32p, C.c_int]
    L.rl_scene_set_camera_matrices.argtypes = [vp, C.c_uint32, C.c_uint32, f32p, f32p]
    L.rl_scene_get_camera_matrices.argtypes = [vp, f32p, f32p, f32p]
    L.rl_scene_set_mesh_emission.argtypes = [vp, C.c_uint32, C.c_int, C.c_float, C.c_int]
    L.rl_scene_override_light_emission.argtypes = [vp, C.c_int, C.c_int]
    L.rl_scene_scale_image.argtypes = [vp, C.c_float]
    L.rl_scene_add_mesh.argtypes = [vp, f32p, C.c_size_t, u32p, C.c_size_t, f32p, f32p, C.POINTER(abi.BsdfDesc), f32p]
    L.rl_scene_add_bitmap.argtypes = [vp, C.c_uint32, C.c_uint32, f32p]
    L.rl_scene_set_medium.argtypes = [vp, f32p, f32p, C.c_int, C.c_float]
    L.rl_scene_build_emitters.argtypes = [vp]
    L.rl_scene_add_point_light.argtypes = [vp, f32p, f32p]
    L.rl_scene_add_directional_light.argtypes = [vp, f32p, f32p]
    L.rl_scene_set_environment.argtypes = [vp, f32p]
    L.rl_scene_set_environment_map.argtypes = [vp, C.c_uint32, C.c_uint32, f32p]
    L.rl_scene_load_pbrt.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.rl_scene_load_mitsuba.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.rl_scene_load.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.rl_scene_image_size.argtypes = [vp, u32p, u32p]
    L.rl_scene_counts.argtypes = [vp, u64p, u64p, u64p]
    L.rl_sampler_seed.argtypes = [C.POINTER(abi.Sampler), C.c_uint64, C.c_int]
    L.rl_sampler_seed.restype = None
    L.rl_sampler_next_u64.argtypes = [C.POINTER(abi.Sampler)]
    L.rl_sampler_next_u64.restype = C.c_uint64
    L.rl_sampler_next_f32.argtypes = [C.POINTER(abi.Sampler)]
    L.rl_sampler_next_f32.restype = C.c_float
    L.rl_path_params_default.argtypes = [C.POINTER(abi.PathParams)]
    L.rl_path_params_default.restype = None
    L.rl_context_create.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.rl_context_destroy.argtypes = [vp]
    L.rl_context_destroy.restype = None
    L.rl_last_error.restype = C.c_char_p
    L.rl_block_count.argtypes = [C.c_uint32, C.c_uint32]
    L.rl_block_count.restype = C.c_size_t
    L.rl_generate_block_seeds.argtypes = [C.POINTER(abi.Sampler), C.c_uint32, C.c_uint32, u64p, C.c_size_t]
    L.rl_render_path.argtypes = [vp, C.POINTER(abi.PathParams), u64p, C.c_size_t, vp, C.c_int, vp, C.POINTER(abi.RenderStats)]
    L.rl_render_path_frames.argtypes = [C.POINTER(vp), C.c_size_t, C.POINTER(abi.PathParams), C.POINTER(u64p), C.c_size_t, C.c_size_t, C.POINTER(C.POINTER(C.c_float)), C.POINTER(abi.RenderStats)]
    L.rl_render_light.argtypes = [vp, C.POINTER(abi.PathParams), u64p, C.c_size_t, vp, C.c_int, vp, C.POINTER(abi.RenderStats)]
    L.rl_vpl_generate.argtypes = [vp, C.POINTER(abi.PathParams), C.c_uint32, C.c_int, C.POINTER(abi.Sampler), C.POINTER(vp), C.POINTER(abi.RenderStats)]
    L.rl_vpl_generate_paths.argtypes = L.rl_vpl_generate.argtypes
    L.rl_vpl_info.argtypes = [vp, u64p, u64p]
    L.rl_vpl_read.argtypes = [vp, u32p, C.c_size_t]
    L.rl_vpl_destroy.argtypes = [vp]
    L.rl_vpl_destroy.restype = None
    L.rl_render_vpl.argtypes = [vp, vp, C.POINTER(abi.PathParams), C.c_int, u64p, C.c_size_t, vp, C.c_int, vp, C.POINTER(abi.RenderStats)]
    L.rl_photon_map_build.argtypes = [vp, vp, C.c_float, C.POINTER(vp)]
    L.rl_photon_map_info.argtypes = [vp, u64p, u64p, u64p, f32p]
    L.rl_photon_map_destroy.argtypes = [vp]
    L.rl_photon_map_destroy.restype = None
    L.rl_render_bre.argtypes = [vp, vp, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, u64p, C.c_size_t, f32p, C.POINTER(abi.RenderStats)]
    L.rl_photon_tree_build.argtypes = [u32p, C.c_size_t, C.c_float, C.c_size_t, C.POINTER(C.c_size_t), f32p, u32p, u32p]
    L.rl_photon_map_build_device.argtypes = [vp, vp, C.c_float, C.POINTER(vp), f32p]
    L.rl_photon_tree_build_device.argtypes = [vp, u32p, C.c_size_t, C.c_float, C.c_size_t, C.POINTER(C.c_size_t), f32p, u32p, u32p]
    L.rl_photon_map_read.argtypes = [vp, C.c_size_t, f32p, u32p, C.c_size_t, f32p]
    L.rl_beam_generate.argtypes = [vp, C.POINTER(abi.PathParams), C.c_uint32, C.POINTER(abi.Sampler), C.POINTER(vp), C.POINTER(abi.RenderStats)]
    L.rl_beam_generate_paths.argtypes = L.rl_beam_generate.argtypes
    L.rl_beam_info.argtypes = [vp, u64p, u64p]
    L.rl_beam_read.argtypes = [vp, u32p, C.c_size_t]
    L.rl_beam_destroy.argtypes = [vp]
    L.rl_beam_destroy.restype = None
    L.rl_beam_split.argtypes = [u32p, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t), u32p]
    L.rl_beam_tree_build.argtypes = [u32p, C.c_size_t, C.c_float, C.c_size_t, C.POINTER(C.c_size_t), f32p, u32p, u32p]
    L.rl_beam_map_build.argtypes = [vp, vp, C.c_float, C.POINTER(vp)]
    L.rl_beam_map_build_words.argtypes = [vp, u32p, C.c_size_t, C.c_uint64, C.c_float, C.POINTER(vp)]
    L.rl_beam_map_info.argtypes = [vp, u64p, u64p, u64p, u64p, f32p]
    L.rl_beam_map_read.argtypes = [vp, C.c_size_t, f32p, u32p, C.c_size_t, f32p]
    L.rl_beam_map_destroy.argtypes = [vp]
    L.rl_beam_map_destroy.restype = None
    L.rl_render_beams.argtypes = [vp, vp, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, u64p, C.c_size_t, f32p, C.POINTER(abi.RenderStats)]
    L.rl_vrl_map_build.argtypes = [vp, vp, C.c_float, C.POINTER(vp)]
    L.rl_vrl_map_build_words.argtypes = [vp, u32p, C.c_size_t, C.c_uint64, C.c_float, C.POINTER(vp)]
    L.rl_vrl_map_info.argtypes = [vp, u64p, u64p, u64p, u64p, u64p, f32p, f32p]
    L.rl_vrl_map_read.argtypes = [vp, C.c_size_t, f32p, u32p, C.c_size_t, f32p, C.c_size_t, f32p]
    L.rl_vrl_map_destroy.argtypes = [vp]
    L.rl_vrl_map_destroy.restype = None
    L.rl_render_vrl.argtypes = L.rl_render_beams.argtypes
    L.rl_pplane_generate.argtypes = [vp, C.POINTER(abi.PathParams), C.c_uint32, C.POINTER(abi.Sampler), C.POINTER(vp), C.POINTER(abi.RenderStats)]
    L.rl_pplane_generate_paths.argtypes = L.rl_pplane_generate.argtypes
    L.rl_pplane_info.argtypes = [vp, u64p, u64p, u64p]
    L.rl_pplane_read.argtypes = [vp, u32p, C.c_size_t, u32p, C.c_size_t]
    L.rl_pplane_destroy.argtypes = [vp]
    L.rl_pplane_destroy.restype = None
    L.rl_pplane_map_build.argtypes = [vp, vp, C.c_float, C.POINTER(vp)]
    L.rl_pplane_map_build_words.argtypes = [vp, u32p, C.c_size_t, u32p, C.c_size_t, C.c_uint64, C.c_float, C.POINTER(vp)]
    L.rl_pplane_map_info.argtypes = [vp, u64p, u64p, u64p, u64p, u64p, u64p, f32p]
    L.rl_pplane_map_read.argtypes = [vp, C.c_int, C.c_size_t, f32p, u32p, C.c_size_t, f32p]
    L.rl_pplane_map_destroy.argtypes = [vp]
    L.rl_pplane_map_destroy.restype = None
    L.rl_render_photon_planes.argtypes = [vp, vp, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, u64p, C.c_size_t, f32p, C.POINTER(abi.RenderStats)]
    L.rl_plane_generate.argtypes = [vp, C.c_uint32, C.c_int, C.POINTER(abi.Sampler), C.POINTER(vp), C.POINTER(abi.RenderStats)]
    L.rl_plane_info.argtypes = [vp, u64p, u64p, C.POINTER(C.c_int)]
    L.rl_plane_read.argtypes = [vp, u32p, C.c_size_t]
    L.rl_plane_destroy.argtypes = [vp]
    L.rl_plane_destroy.restype = None
    L.rl_plane_tree_build.argtypes = [u32p, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t), f32p, u32p, u32p]
    L.rl_plane_map_build.argtypes = [vp, vp, C.POINTER(vp)]
    L.rl_plane_generate_lanes.argtypes = L.rl_plane_generate.argtypes
    L.rl_plane_map_build_device.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(C.c_float)]
    L.rl_plane_tree_build_device.argtypes = [vp, u32p, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t), f32p, u32p, u32p]
    L.rl_plane_map_info.argtypes = [vp, u64p, u64p, u64p, C.POINTER(C.c_int)]
    L.rl_plane_map_read.argtypes = [vp, C.c_size_t, f32p, u32p, C.c_size_t, f32p]
    L.rl_plane_map_destroy.argtypes = [vp]
    L.rl_plane_map_destroy.restype = None
    L.rl_render_plane_single.argtypes = [vp, vp, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, u64p, C.c_size_t, f32p, C.POINTER(abi.RenderStats)]
    L.rl_render_plane_uncorrelated.argtypes = [vp, C.c_uint32, C.c_int, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, u64p, C.c_size_t, f32p, C.POINTER(abi.RenderStats)]
    L.rl_point_normal_params_default.argtypes = [C.POINTER(PointNormalParams)]
    L.rl_point_normal_params_default.restype = None
    L.rl_render_point_normal.argtypes = [vp, C.POINTER(PointNormalParams), u64p, C.c_size_t, f32p, C.POINTER(abi.RenderStats)]
    L.rl_point_normal_mis_params_default.argtypes = [C.POINTER(PointNormalMisParams)]
    L.rl_point_normal_mis_params_default.restype = None
    L.rl_render_point_normal_mis.argtypes = [vp, C.POINTER(PointNormalMisParams), u64p, C.c_size_t, f32p, C.POINTER(abi.RenderStats)]
    L.rl_point_normal_taylor_params_default.argtypes = [C.POINTER(PointNormalTaylorParams)]
    L.rl_point_normal_taylor_params_default.restype = None
    L.rl_render_point_normal_taylor.argtypes = [vp, C.POINTER(PointNormalTaylorParams), u64p, C.c_size_t, f32p, C.POINTER(abi.RenderStats)]
    L.rl_point_normal_ats_params_default.argtypes = [C.POINTER(PointNormalAtsParams)]
    L.rl_point_normal_ats_params_default.restype = None
    L.rl_render_point_normal_ats.argtypes = [vp, C.POINTER(PointNormalAtsParams), u64p, C.c_size_t, f32p, C.POINTER(abi.RenderStats)]
    for fn in (L.rl_render_ao, L.rl_render_direct):
        fn.argtypes = [vp, C.POINTER(abi.McParams), u64p, C.c_size_t, vp, C.c_int, vp, C.POINTER(abi.RenderStats)]
    L.rl_multi_create.argtypes = [vp, C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
    L.rl_multi_destroy.argtypes = [vp]
    L.rl_multi_destroy.restype = None
    L.rl_multi_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.rl_multi_render_path.argtypes = [vp, C.POINTER(abi.PathParams), u64p, C.c_size_t, vp, C.POINTER(abi.RenderStats)]
    L.rl_multi_describe.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.rl_multi_shard_stats.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(abi.RenderStats)]
    L.rl_trace_batch.argtypes = [vp, C.c_size_t, f32p, f32p, f32p, f32p, f32p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.rl_visible_batch.argtypes = [vp, C.c_size_t, f32p, f32p, C.POINTER(C.c_uint8)]
    for fn in (L.rl_save_pfm, L.rl_save_png, L.rl_save_exr, L.rl_save_image):
        fn.argtypes = [C.c_char_p, f32p, C.c_uint32, C.c_uint32]
    L.rl_build_info.restype = C.c_char_p
    # test hooks
    L.rl_debug_numerics.argtypes = [C.c_int, C.c_size_t, f32p, f32p, f32p]
    L.rl_debug_math_sweep.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_size_t, f32p, C.c_size_t, C.c_int, f32p]
    L.rl_debug_bvh.argtypes = [vp, u64p, u64p, f32p, u64p, u64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.rl_debug_bvh_sizes.argtypes = [vp, u64p, u64p, u32p, C.POINTER(C.c_int)]
    L.rl_debug_camera_ray.argtypes = [vp, C.c_float, C.c_float, f32p, f32p]
    _lib = L
    return L


def _check(rc):
    if rc < 0:
        msg = (lib().rl_last_error() or b"").decode("utf-8", "replace")
        raise (NoDeviceError if rc == RL_ERR_NO_DEVICE else RustlightError)(rc, msg)
    return rc


class IndependentSampler:
    """IndependentSampler { rnd: SmallRng::seed_from_u64(seed) } (examples/cli.rs:886-890)."""

    def __init__(self, seed: int, variant: int = 0):
        self.s = abi.Sampler()
        self.variant = variant
        lib().rl_sampler_seed(C.byref(self.s), seed, variant)

    def next(self) -> float:
        return float(lib().rl_sampler_next_f32(C.byref(self.s)))

    def next_u64(self) -> int:
        return int(lib().rl_sampler_next_u64(C.byref(self.s)))

    def block_seeds(self, width: int, height: int) -> np.ndarray:
        """generate_img_blocks: one clone_box seed per 16x16 block, x-major (integrators/mod.rs:357-371)."""
        n = lib().rl_block_count(width, height)
        seeds = np.zeros(n, dtype=np.uint64)
        _check(lib().rl_generate_block_seeds(C.byref(self.s), width, height, abi.u64ptr(seeds), n))
        return seeds


class Scene:
    """Host-side flattened `Scene` (src/scene.rs:16-30)."""

    def __init__(self, sd: Optional[S.SceneData] = None, handle=None, camera_matrices=None):
        """camera_matrices = (sample_to_camera, to_world), column-major 16-vectors: the camera as rustlight's `Camera` holds it
        (rl_scene_set_camera_matrices) instead of Camera::new's arguments."""
        L = lib()
        self.sd = sd
        if handle is not None:
            self.h = handle
        else:
            h = C.c_void_p()
            _check(L.rl_scene_create(C.byref(h)))
            self.h = h
            tw = np.ascontiguousarray(sd.to_world, dtype=np.float32)
            if camera_matrices is not None:
                stc, twm = (np.ascontiguousarray(m, dtype=np.float32).ravel() for m in camera_matrices)
                _check(L.rl_scene_set_camera_matrices(self.h, sd.width, sd.height, abi.fptr(stc), abi.fptr(twm)))
            else:
                _check(L.rl_scene_set_camera(self.h, sd.width, sd.height, sd.fov, sd.fov_axis, abi.fptr(tw), int(sd.flip)))
            for (w, hgt, rgb) in sd.bitmaps:
                a = np.ascontiguousarray(rgb, dtype=np.float32)
                _check(L.rl_scene_add_bitmap(self.h, w, hgt, abi.fptr(a)))
            for k, m in enumerate(sd.meshes):
                v, i, n, uv, e = abi.mesh_arrays(m)
                bd = abi.bsdf_desc(m.bsdf)
                _check(L.rl_scene_add_mesh(self.h, abi.fptr(v), v.shape[0], abi.u32ptr(i), i.shape[0], abi.fptr(n),
                                           abi.fptr(uv), C.byref(bd), abi.fptr(e)))
                if getattr(m, "emission_kind", None):          # EmissionType::HSV / Texture
                    ek = m.emission_kind
                    _check(L.rl_scene_set_mesh_emission(self.h, k, 1 if ek[0] == "hsv" else 2, float(ek[1]), int(ek[2]) if len(ek) > 2 else -1))
            if sd.medium is not None:
                sa = np.asarray(sd.medium.sigma_a, dtype=np.float32)
                ss = np.asarray(sd.medium.sigma_s, dtype=np.float32)
                _check(L.rl_scene_set_medium(self.h, abi.fptr(sa), abi.fptr(ss), sd.medium.phase, sd.medium.g))
            for lt in sd.lights:
                a = np.asarray(lt["a"], np.float32)
                b = np.asarray(lt["intensity"], np.float32)
                fn = L.rl_scene_add_point_light if lt["type"] == "point" else L.rl_scene_add_directional_light
                _check(fn(self.h, abi.fptr(a), abi.fptr(b)))
            if sd.environment is not None:
                e = np.asarray(sd.environment, np.float32)
                _check(L.rl_scene_set_environment(self.h, abi.fptr(e)))
            if sd.environment_map is not None:
                em = np.ascontiguousarray(sd.environment_map, np.float32)
                _check(L.rl_scene_set_environment_map(self.h, em.shape[1], em.shape[0], abi.fptr(em)))
        if sd is not None and getattr(sd, "use_ats", False):
            _check(L.rl_scene_enable_ats(self.h, 1))
        _check(L.rl_scene_build_emitters(self.h))

    def camera_matrices(self):
        """(sample_to_camera[16], to_world[16], position[3]) the scene's camera uses, column-major."""
        a, b, c = np.zeros(16, np.float32), np.zeros(16, np.float32), np.zeros(3, np.float32)
        _check(lib().rl_scene_get_camera_matrices(self.h, abi.fptr(a), abi.fptr(b), abi.fptr(c)))
        return a, b, c

    @classmethod
    def from_desc(cls, sd: S.SceneData, camera_matrices=None) -> "Scene":
        """The same scene through the one-call POD entry (rl_scene_create_from_desc, SURVEY §8(b) "SceneDesc"); camera_matrices as in __init__."""
        keep = []                                  # numpy arrays must outlive the call
        def fp(a):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float32); keep.append(a)
            return abi.fptr(a)
        d = abi.SceneDesc()
        d.width, d.height, d.fov_degrees, d.fov_axis, d.flip = sd.width, sd.height, sd.fov, sd.fov_axis, int(sd.flip)
        d.to_world = (C.c_float * 16)(*np.asarray(sd.to_world, np.float32).ravel())
        if camera_matrices is not None:
            d.has_camera_matrices = 1
            d.sample_to_camera = (C.c_float * 16)(*np.asarray(camera_matrices[0], np.float32).ravel())
            d.to_world = (C.c_float * 16)(*np.asarray(camera_matrices[1], np.float32).ravel())
            d.fov_degrees, d.fov_axis, d.flip = 0.0, 0, 0
        meshes = (abi.MeshDesc * max(1, len(sd.meshes)))()
        for k, m in enumerate(sd.meshes):
            v, i, n, uv, e = abi.mesh_arrays(m)
            keep.extend([v, i])
            meshes[k].vertices, meshes[k].n_vertices = abi.fptr(v), v.shape[0]
            meshes[k].indices, meshes[k].n_triangles = abi.u32ptr(i), i.shape[0]
            meshes[k].normals, meshes[k].uv = fp(n), fp(uv)
            meshes[k].bsdf = abi.bsdf_desc(m.bsdf)
            if e is not None:
                meshes[k].has_emission = 1
                meshes[k].emission_rgb = (C.c_float * 3)(*e)
            if getattr(m, "emission_kind", None):
                ek = m.emission_kind
                meshes[k].emission_type, meshes[k].emission_scale, meshes[k].emission_bitmap_id = (1 if ek[0] == "hsv" else 2), float(ek[1]), (int(ek[2]) if len(ek) > 2 else -1)
        d.meshes, d.n_meshes = meshes, len(sd.meshes)
        bitmaps = (abi.BitmapDesc * max(1, len(sd.bitmaps)))()
        for k, (w, h, rgb) in enumerate(sd.bitmaps):
            bitmaps[k].width, bitmaps[k].height, bitmaps[k].rgb = w, h, fp(rgb)
        d.bitmaps, d.n_bitmaps = bitmaps, len(sd.bitmaps)
        lights = (abi.LightDesc * max(1, len(sd.lights)))()
        for k, lt in enumerate(sd.lights):
            lights[k].kind = 0 if lt["type"] == "point" else 1
            lights[k].a = (C.c_float * 3)(*lt["a"])
            lights[k].intensity = (C.c_float * 3)(*lt["intensity"])
        d.lights, d.n_lights = lights, len(sd.lights)
        if sd.environment is not None:
            d.has_environment = 1
            d.environment_rgb = (C.c_float * 3)(*sd.environment)
        if sd.environment_map is not None:
            em = np.ascontiguousarray(sd.environment_map, np.float32); keep.append(em)
            d.env_map_width, d.env_map_height, d.env_map_rgb = em.shape[1], em.shape[0], abi.fptr(em)
        if sd.medium is not None:
            d.has_medium = 1
            d.sigma_a = (C.c_float * 3)(*sd.medium.sigma_a)
            d.sigma_s = (C.c_float * 3)(*sd.medium.sigma_s)
            d.phase_type, d.g = sd.medium.phase, sd.medium.g
        d.build_ats = int(bool(getattr(sd, "use_ats", False)))
        h = C.c_void_p()
        _check(lib().rl_scene_create_from_desc(C.byref(d), C.byref(h)))
        obj = cls.__new__(cls)
        obj.sd, obj.h = sd, h
        return obj

    @classmethod
    def load_pbrt(cls, path: str, use_shading_normals: bool = True) -> "Scene":
        h = C.c_void_p()
        _check(lib().rl_scene_load_pbrt(path.encode(), int(use_shading_normals), C.byref(h)))
        return cls(None, handle=h)

    @classmethod
    def load_mitsuba(cls, path: str, use_shading_normals: bool = True) -> "Scene":
        h = C.c_void_p()
        _check(lib().rl_scene_load_mitsuba(path.encode(), int(use_shading_normals), C.byref(h)))
        return cls(None, handle=h)

    @classmethod
    def load(cls, path: str, use_shading_normals: bool = True) -> "Scene":
        """SceneLoaderManager::load: .pbrt or .xml by extension (src/scene_loader.rs:27-58)."""
        h = C.c_void_p()
        _check(lib().rl_scene_load(path.encode(), int(use_shading_normals), C.byref(h)))
        return cls(None, handle=h)

    def set_medium(self, sigma_a, sigma_s, phase=S.PHASE_ISOTROPIC, g=0.0):
        sa = np.asarray(sigma_a, dtype=np.float32)
        ss = np.asarray(sigma_s, dtype=np.float32)
        _check(lib().rl_scene_set_medium(self.h, abi.fptr(sa), abi.fptr(ss), phase, g))

    def __del__(self):
        try:
            lib().rl_scene_destroy(self.h)
        except Exception:
            pass

    @property
    def size(self):
        w, h = C.c_uint32(), C.c_uint32()
        _check(lib().rl_scene_image_size(self.h, C.byref(w), C.byref(h)))
        return w.value, h.value

    def counts(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().rl_scene_counts(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"meshes": a.value, "triangles": b.value, "emitters": c.value}

    def debug_bvh(self):
        nn, npr = C.c_uint64(), C.c_uint64()
        _check(lib().rl_debug_bvh(self.h, C.byref(nn), C.byref(npr), None, None, None, None, None))
        boxes = np.zeros((nn.value, 6), np.float32)
        info = np.zeros(nn.value, np.uint64)
        count = np.zeros(nn.value, np.uint64)
        pm = np.zeros(npr.value, np.int32)
        pt = np.zeros(npr.value, np.int32)
        _check(lib().rl_debug_bvh(self.h, C.byref(nn), C.byref(npr), abi.fptr(boxes), abi.u64ptr(info), abi.u64ptr(count),
                                  pm.ctypes.data_as(C.POINTER(C.c_int32)), pt.ctypes.data_as(C.POINTER(C.c_int32))))
        return boxes, info, count, pm, pt

    def debug_emitters_cdf(self):
        n = C.c_uint64(0)
        L = lib()
        L.rl_debug_emitters_cdf.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
        _check(L.rl_debug_emitters_cdf(self.h, C.byref(n), None))
        out = np.zeros(n.value, np.float32)
        _check(L.rl_debug_emitters_cdf(self.h, C.byref(n), abi.fptr(out)))
        return out

    def debug_ats(self):
        """(nodes [n, 16] f32 — struct LightNode, link words are int32 bit patterns —, light_emitter, light_prim)."""
        L = lib()
        i32p = C.POINTER(C.c_int32)
        L.rl_debug_ats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.POINTER(C.c_uint64), i32p, i32p]
        nn, nl = C.c_uint64(), C.c_uint64()
        _check(L.rl_debug_ats(self.h, C.byref(nn), None, C.byref(nl), None, None))
        nodes = np.zeros((nn.value, 16), np.float32); le = np.zeros(nl.value, np.int32); lp = np.zeros(nl.value, np.int32)
        _check(L.rl_debug_ats(self.h, C.byref(nn), abi.fptr(nodes), C.byref(nl), le.ctypes.data_as(i32p), lp.ctypes.data_as(i32p)))
        return nodes, le, lp

    def debug_ats_angles(self):
        """[n, 2] f32: LightBounds::theta_o, theta_e of debug_ats' nodes, as the host tree stores them (LightNode keeps their cosines)."""
        L = lib()
        L.rl_debug_ats_angles.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
        nn = C.c_uint64()
        _check(L.rl_debug_ats_angles(self.h, C.byref(nn), None))
        angles = np.zeros((nn.value, 2), np.float32)
        _check(L.rl_debug_ats_angles(self.h, C.byref(nn), abi.fptr(angles)))
        return angles

    def camera_ray(self, px, py):
        o = (C.c_float * 3)()
        d = (C.c_float * 3)()
        _check(lib().rl_debug_camera_ray(self.h, px, py, o, d))
        return np.array(o[:], np.float32), np.array(d[:], np.float32)


def path_params(spp=1, min_depth=0, max_depth=None, rr_depth=0, strategy=STRATEGY_ALL, single_scattering=False,
                stream_mode=STREAM_PER_SAMPLE, seed_variant=0, shard_index=0, shard_count=1, pool_slots=0, pipeline=0, sample_split=0, numerics=0) -> abi.PathParams:
    """rl_path_params for the tests and bench.py.  NOTE the default stream mode: this helper defaults to the throughput decomposition
    (STREAM_PER_SAMPLE), which most parity tests exercise; the plugin-level surfaces — rl_path_params_default, the C++ / Python
    IntegratorPathTracing, the CLI — default to rustlight's own RL_STREAM_REFERENCE_ORDER."""
    p = abi.PathParams()
    lib().rl_path_params_default(C.byref(p))
    p.spp = spp
    p.has_min_depth, p.min_depth = (0, 0) if min_depth is None else (1, min_depth)
    p.has_max_depth, p.max_depth = (0, 0) if max_depth is None else (1, max_depth)
    p.has_rr_depth, p.rr_depth = (0, 0) if rr_depth is None else (1, rr_depth)
    p.strategy = strategy
    p.single_scattering = int(single_scattering)
    p.stream_mode = stream_mode
    p.seed_variant = seed_variant
    p.shard_index, p.shard_count = shard_index, shard_count
    p.pool_slots = pool_slots
    p.pipeline = pipeline
    p.sample_split = sample_split
    p.numerics = numerics
    return p


class _ImageCalls:
    """What Context and MultiContext share: the call that fills one image of the owner's width x height."""

    def _image_call(self, seeds, call, out=None):
        """One ABI call that renders an image: call(seeds pointer, n, image pointer, stats reference) -> rc.  Returns (image HxWx3 f32, abi.RenderStats); with
        `out`, a pointer of the caller's, the image goes there and None comes back for it."""
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        st = abi.RenderStats()
        img = np.zeros((self.height, self.width, 3), dtype=np.float32) if out is None else None
        _check(call(abi.u64ptr(seeds), seeds.shape[0], abi.fptr(img) if out is None else out, C.byref(st)))
        return img, st


class Context(_ImageCalls):
    """Device context = BVHAccel::new(scene) + the scene uploaded to one MI355X."""

    def __init__(self, scene: Scene, device: int = 0):
        self.scene = scene
        self.device = device
        h = C.c_void_p()
        _check(lib().rl_context_create(scene.h, device, C.byref(h)))
        self.h = h
        self.width, self.height = scene.size

    def close(self):
        if getattr(self, "h", None):
            lib().rl_context_destroy(self.h)
            self.h = None

    def set_option(self, name: str, value=None):
        """rl_context_set_option: an execution option of this context (csrc/kernels/knobs.h: "spec_force", "no_overlap", "state_budget_mb", ...; none changes a
        result), `None` = back to the default.  The context took the environment's RL_<NAME> values when it was created; renders never read the environment."""
        _check(lib().rl_context_set_option(self.h, name.lower().encode(), None if value is None else str(value).encode()))

    def sample_buf_bytes(self) -> int:
        """Test hook (rl_debug_sample_buf_bytes): bytes of the per-sample parking buffer this context holds (0 until a render needed one)."""
        n = C.c_uint64(0)
        fn = lib().rl_debug_sample_buf_bytes
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        _check(fn(self.h, C.byref(n)))
        return int(n.value)

    def get_option(self, name: str):
        v = lib().rl_context_get_option(self.h, name.lower().encode())
        return None if v is None else v.decode()

    @contextlib.contextmanager
    def options(self, **kw):
        """`with ctx.options(spec_force=1, no_overlap=1): ...` — the options set inside the block, back to what they were after it."""
        before = {k: self.get_option(k) for k in kw}
        try:
            for k, v in kw.items():
                self.set_option(k, v)
            yield self
        finally:
            for k, v in before.items():
                self.set_option(k, v)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def render(self, seeds: np.ndarray, params: abi.PathParams, out_device_ptr: Optional[int] = None, stream: Optional[int] = None, out_host_ptr: Optional[int] = None):
        """Integrator::compute.  Returns (image HxWx3 f32 | None when rendering into a device pointer or a caller's (e.g. pinned) host buffer, stats dict)."""
        on_device = out_host_ptr is None and out_device_ptr is not None
        ptr = out_device_ptr if on_device else out_host_ptr
        img, st = self._image_call(seeds, lambda sp, n, out, st: lib().rl_render_path(self.h, C.byref(params), sp, n, out, int(on_device), C.c_void_p(stream) if stream else None, st),
                                   None if ptr is None else C.c_void_p(ptr))
        return img, st.as_dict()

    def _render_mc(self, fn, seeds, spp=1, stream_mode=STREAM_PER_SAMPLE, seed_variant=0, shard_index=0, shard_count=1,
                   max_distance=1.0, normal_correction=False, nb_bsdf_samples=1, nb_light_samples=1):
        p = abi.McParams()
        p.spp, p.stream_mode, p.seed_variant, p.shard_index, p.shard_count = spp, stream_mode, seed_variant, shard_index, shard_count
        p.has_max_distance, p.max_distance = (0, 0.0) if max_distance is None else (1, max_distance)
        p.normal_correction = int(normal_correction)
        p.nb_bsdf_samples, p.nb_light_samples = nb_bsdf_samples, nb_light_samples
        img, st = self._image_call(seeds, lambda sp, n, out, st: fn(self.h, C.byref(p), sp, n, out, 0, None, st))
        return img, st.as_dict()

    def render_ao(self, seeds, **kw):
        """IntegratorAO { max_distance, normal_correction } (src/integrators/ao.rs)."""
        return self._render_mc(lib().rl_render_ao, seeds, **kw)

    def render_direct(self, seeds, **kw):
        """IntegratorDirect { nb_bsdf_samples, nb_light_samples } (src/integrators/direct.rs)."""
        return self._render_mc(lib().rl_render_direct, seeds, **kw)

    def render_light(self, seeds, spp=1, min_depth=0, max_depth=None, rr_depth=0, strategy=LIGHT_ALL, seed_variant=0, stream_mode=STREAM_PER_SAMPLE,
                     numerics=NUMERICS_EXACT, shard_count=1):
        """IntegratorLightTracing (src/integrators/explicit/light.rs) through rl_render_light: (image HxWx3 f32, stats dict).  stats: camera_samples = light
        paths, shadow_rays = camera connections, reserved[0..2] = splats added / dropped as invalid / saturated.  stream_mode, numerics and shard_count only
        take the values the C ABI accepts (anything else is RL_ERR_UNSUPPORTED)."""
        p = path_params(spp, min_depth, max_depth, rr_depth, strategy, False, stream_mode, seed_variant, shard_count=shard_count, numerics=numerics)
        img, st = self._image_call(seeds, lambda sp, n, out, st: lib().rl_render_light(self.h, C.byref(p), sp, n, out, 0, None, st))
        d = st.as_dict()
        d["splats"], d["splats_invalid"], d["splats_saturated"] = (int(v) for v in st.reserved[:3])
        return img, d

    def _light_pass(self, name, set_class, sampler, nb, max_depth, rr_depth, streams, *option):
        """rl_<name>_generate (streams="reference") or rl_<name>_generate_paths ("per_path") behind vpl_generate, beam_generate and pplane_generate:
        (set_class handle, stats dict).  `option`: what the call takes between the count and the sampler."""
        if streams not in LIGHT_STREAMS:
            raise ValueError(f"streams must be one of {LIGHT_STREAMS}, not {streams!r}")
        p = path_params(1, 0, max_depth, rr_depth, stream_mode=STREAM_REFERENCE_ORDER, seed_variant=sampler.variant)
        st = abi.RenderStats()
        h = C.c_void_p()
        fn = getattr(lib(), f"rl_{name}_generate" if streams == "reference" else f"rl_{name}_generate_paths")
        _check(fn(self.h, C.byref(p), nb, *option, C.byref(sampler.s), C.byref(h), C.byref(st)))
        d = st.as_dict()
        if streams == "per_path":
            d["paths_walked"] = int(st.reserved[0])
        return set_class(h, self), d

    def vpl_generate(self, sampler: "IndependentSampler", nb_vpl=128, max_depth=None, rr_depth=0, option_vpl=VPL_ALL, streams="reference"):
        """IntegratorVPL's generation (vpl.rs:182-210): (VplSet, stats dict).  streams="reference": rl_vpl_generate, one lane on the main sampler's serial stream,
        seed for seed the reference; `sampler` is advanced as the reference's main sampler is.  streams="per_path": rl_vpl_generate_paths, one light path per lane
        on the stream of the k-th clone_box of `sampler` (include/rustlight_amd.h has the contract): statistically, not seed-for-seed, the
        same image; `sampler` is advanced by one next_u64 per kept path.  stats: camera_samples = light paths shot (kept), vertices, extension_rays, rng_draws,
        ms_prepass = the generation kernels' time; per_path adds iterations = rounds and paths_walked = reserved[0]."""
        return self._light_pass("vpl", VplSet, sampler, nb_vpl, max_depth, rr_depth, streams, option_vpl)

    def render_vpl(self, vpls: "VplSet", seeds, spp=1, option_lt=VPL_ALL, seed_variant=0, shard_index=0, shard_count=1, stream_mode=STREAM_REFERENCE_ORDER,
                   numerics=NUMERICS_EXACT):
        """IntegratorVPL's gather (vpl.rs:212-535) through rl_render_vpl: (image HxWx3 f32, stats dict).  stats: shadow_rays = connection rays traced,
        gather_surface / gather_volume = reserved[0] / reserved[1], ms_raygen = primary passes, ms_other = gather passes."""
        p = path_params(spp, 0, None, 0, stream_mode=stream_mode, seed_variant=seed_variant, shard_index=shard_index, shard_count=shard_count, numerics=numerics)
        img, st = self._image_call(seeds, lambda sp, n, out, st: lib().rl_render_vpl(self.h, vpls.h, C.byref(p), option_lt, sp, n, out, 0, None, st))
        d = st.as_dict()
        d["gather_surface"], d["gather_volume"] = int(st.reserved[0]), int(st.reserved[1])
        return img, d

    def _map(self, fn, map_class, *args, after=()):
        """fn(context, *args, &handle, *after) behind the *_map and *_map_from_words methods: the map_class over the handle."""
        h = C.c_void_p()
        _check(fn(self.h, *args, C.byref(h), *after))
        return map_class(h, self)

    def _timed_map(self, name, map_class, build, records, *args):
        """photon_map / plane_map: the map from <name>(context, records, *args, &handle) or, build="device", <name>_device(.., &handle, &ms) — with ms_build,
        the wall clock of the call, and ms_kernels, the device build's kernel time (None: host).  `build` is checked before anything else is touched."""
        if build not in TREE_BUILDS:
            raise ValueError(f"build must be one of {TREE_BUILDS}, not {build!r}")
        ms = C.c_float(0.0)
        t0 = time.perf_counter()
        if build == "device":
            m = self._map(getattr(lib(), name + "_device"), map_class, records.h, *args, after=(C.byref(ms),))
        else:
            m = self._map(getattr(lib(), name), map_class, records.h, *args)
        m.ms_build = (time.perf_counter() - t0) * 1e3
        m.ms_kernels = float(ms.value) if build == "device" else None
        return m

    def photon_map(self, vpls: "VplSet", radius=PHOTON_RADIUS_DEFAULT, build="host"):
        """rl_photon_map_build: the photon tree of the beam radiance estimate over a set generated with option_vpl = VPL_VOLUME (its records are the reference's
        photons).  radius: the reference hard-codes PHOTON_RADIUS_DEFAULT.  build="device": rl_photon_map_build_device, the same map byte for byte from device
        kernels, no record leaving the GPU.  PhotonMap.ms_build: wall clock of the call; PhotonMap.ms_kernels: the device build's kernel time (None: host)."""
        return self._timed_map("rl_photon_map_build", PhotonMap, build, vpls, radius)

    def photon_tree_build_device(self, words, radius):
        """rl_photon_tree_build_device: photon_tree_build's arrays, computed by the kernels of the device build on this context's device."""
        w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, VPL_WORDS)
        return _tree_arrays(lambda *out: lib().rl_photon_tree_build_device(self.h, abi.u32ptr(w), w.shape[0], radius, *out), w.shape[0])

    def _render_gather(self, fn, handle, seeds, spp, seed_variant, shard_index, shard_count, names):
        """rl_render_bre / rl_render_plane_single: (image HxWx3 f32, stats dict with reserved[k] under names[k])."""
        img, st = self._image_call(seeds, lambda sp, n, out, st: fn(self.h, handle, spp, seed_variant, shard_index, shard_count, sp, n, out, st))
        d = st.as_dict()
        d.update((name, int(st.reserved[k])) for k, name in enumerate(names))
        return img, d

    def render_bre(self, photons: "PhotonMap", seeds, spp=1, seed_variant=0, shard_index=0, shard_count=1):
        """The beam radiance estimate's gather (vol_primitives.rs:712-790) through rl_render_bre: (image HxWx3 f32, stats dict).  stats: nodes_entered /
        photons_gathered = reserved[0] / reserved[1], ms_other = the gather kernel."""
        return self._render_gather(lib().rl_render_bre, photons.h, seeds, spp, seed_variant, shard_index, shard_count, ("nodes_entered", "photons_gathered"))

    def beam_generate(self, sampler: "IndependentSampler", nb_primitive=128, max_depth=None, rr_depth=0, streams="reference"):
        """The photon beams' beam pass (vol_primitives.rs:437-523, 608-630): (BeamSet, stats dict).  streams="reference": rl_beam_generate, one lane on the main
        sampler's serial stream, seed for seed the reference; streams="per_path": rl_beam_generate_paths under rl_vpl_generate_paths' stream contract.  `sampler`
        and the stats follow Context.vpl_generate's rules."""
        return self._light_pass("beam", BeamSet, sampler, nb_primitive, max_depth, rr_depth, streams)

    def beam_map(self, beams: "BeamSet", radius=PHOTON_RADIUS_DEFAULT):
        """rl_beam_map_build: the beams of a set split into sub-beams and sorted into the beam tree on the host, uploaded.  radius: the reference hard-codes
        PHOTON_RADIUS_DEFAULT."""
        return self._map(lib().rl_beam_map_build, BeamMap, beams.h, radius)

    def beam_map_from_words(self, words, n_paths, radius=PHOTON_RADIUS_DEFAULT):
        """rl_beam_map_build_words: Context.beam_map over caller-supplied beam records ([n, BEAM_WORDS] u32) of n_paths light paths."""
        w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, BEAM_WORDS)
        return self._map(lib().rl_beam_map_build_words, BeamMap, abi.u32ptr(w), w.shape[0], n_paths, radius)

    def render_beams(self, beams: "BeamMap", seeds, spp=1, seed_variant=0, shard_index=0, shard_count=1):
        """The photon beams' gather (vol_primitives.rs:140-199, 705-790) through rl_render_beams: (image HxWx3 f32, stats dict).  stats: nodes_entered /
        beams_accepted = reserved[0] / reserved[1], ms_other = the gather kernel."""
        return self._render_gather(lib().rl_render_beams, beams.h, seeds, spp, seed_variant, shard_index, shard_count, ("nodes_entered", "beams_accepted"))

    def vrl_map(self, beams: "BeamSet", radius=PHOTON_RADIUS_DEFAULT):
        """rl_vrl_map_build: the beams of a beam pass partitioned by from_surface — the surface beams split and sorted into the beam tree, the others kept in
        storing order as VRLs with their roulette probabilities — and uploaded."""
        return self._map(lib().rl_vrl_map_build, VrlMap, beams.h, radius)

    def vrl_map_from_words(self, words, n_paths, radius=PHOTON_RADIUS_DEFAULT):
        """rl_vrl_map_build_words: Context.vrl_map over caller-supplied beam records ([n, BEAM_WORDS] u32) of n_paths light paths."""
        w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, BEAM_WORDS)
        return self._map(lib().rl_vrl_map_build_words, VrlMap, abi.u32ptr(w), w.shape[0], n_paths, radius)

    def render_vrl(self, vmap: "VrlMap", seeds, spp=1, seed_variant=0, shard_index=0, shard_count=1):
        """The virtual ray lights' gather (vol_primitives.rs:201-253, 741-764) through rl_render_vrl: (image HxWx3 f32, stats dict).  stats: nodes_entered /
        beams_accepted / vrl_accepted / vrl_visible = reserved[0 .. 3], ms_prepass = the chain pass, ms_other = both kernels."""
        return self._render_gather(lib().rl_render_vrl, vmap.h, seeds, spp, seed_variant, shard_index, shard_count,
                                   ("nodes_entered", "beams_accepted", "vrl_accepted", "vrl_visible"))

    def pplane_generate(self, sampler: "IndependentSampler", nb_primitive=128, max_depth=None, rr_depth=0, streams="reference"):
        """The photon planes' plane pass (vol_primitives.rs:376-523, 608-630): (PPlaneSet, stats dict).  The light paths of Context.beam_generate, stored as
        surface beams and planes while fewer than nb_primitive planes are stored.  streams, `sampler` and the stats follow Context.beam_generate's rules."""
        return self._light_pass("pplane", PPlaneSet, sampler, nb_primitive, max_depth, rr_depth, streams)

    def pplane_map(self, records: "PPlaneSet", radius=PHOTON_RADIUS_DEFAULT):
        """rl_pplane_map_build: the surface beams of a set split and sorted into the beam tree, its planes sorted into the plane tree, both uploaded.  The plane
        tree is built on the host, or by the device kernels under the context option pplane_tree_device = 1 (the same bytes)."""
        return self._map(lib().rl_pplane_map_build, PPlaneMap, records.h, radius)

    def pplane_map_from_words(self, beam_words, plane_words, n_paths, radius=PHOTON_RADIUS_DEFAULT):
        """rl_pplane_map_build_words: Context.pplane_map over caller-supplied beam ([n, BEAM_WORDS] u32) and plane ([m, PLANE_WORDS] u32) records of n_paths
        light paths."""
        b = np.ascontiguousarray(beam_words, dtype=np.uint32).reshape(-1, BEAM_WORDS)
        w = np.ascontiguousarray(plane_words, dtype=np.uint32).reshape(-1, PLANE_WORDS)
        return self._map(lib().rl_pplane_map_build_words, PPlaneMap, abi.u32ptr(b), b.shape[0], abi.u32ptr(w), w.shape[0], n_paths, radius)

    def render_photon_planes(self, pmap: "PPlaneMap", seeds, spp=1, seed_variant=0, shard_index=0, shard_count=1):
        """The photon planes' gather (vol_primitives.rs:295-373, 705-790) through rl_render_photon_planes: (image HxWx3 f32, stats dict).  stats: nodes_entered
        (both trees) / beams_accepted / planes_intersected / planes_visible = reserved[0 .. 3], ms_other = the gather kernel."""
        return self._render_gather(lib().rl_render_photon_planes, pmap.h, seeds, spp, seed_variant, shard_index, shard_count,
                                   ("nodes_entered", "beams_accepted", "planes_intersected", "planes_visible"))

    def plane_generate(self, sampler: "IndependentSampler", nb_primitive=128, strategy="average", form="serial"):
        """IntegratorSinglePlane's plane pass (plane_single.rs:363-427) through rl_plane_generate: (PlaneSet, stats dict).  `sampler` is advanced as the
        reference's main sampler is.  stats: camera_samples = iterations (number_plane_gen), vertices = planes, rng_draws, ms_prepass = the kernel.
        form="lanes": rl_plane_generate_lanes, one lane per iteration, the same set, sampler and counters; its records stay on the device."""
        if form not in PLANE_FORMS:
            raise ValueError(f"form must be one of {PLANE_FORMS}, not {form!r}")
        st = abi.RenderStats()
        h = C.c_void_p()
        fn = lib().rl_plane_generate_lanes if form == "lanes" else lib().rl_plane_generate
        _check(fn(self.h, nb_primitive, plane_strategy(strategy), C.byref(sampler.s), C.byref(h), C.byref(st)))
        return PlaneSet(h, self), st.as_dict()

    def plane_map(self, planes: "PlaneSet", build="host"):
        """rl_plane_map_build: the plane tree over a generated set, built on the host and uploaded.  build="device": rl_plane_map_build_device, the same map
        byte for byte from device kernels.  PlaneMap.ms_build: wall clock of the call, ms; PlaneMap.ms_kernels: the device build's kernel time (None: host)."""
        return self._timed_map("rl_plane_map_build", PlaneMap, build, planes)

    def plane_tree_build_device(self, words):
        """rl_plane_tree_build_device: plane_tree_build's arrays, computed by the kernels of the device build on this context's device."""
        w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, PLANE_WORDS)
        return _tree_arrays(lambda *out: lib().rl_plane_tree_build_device(self.h, abi.u32ptr(w), w.shape[0], *out), w.shape[0])

    def render_plane_single(self, planes: "PlaneMap", seeds, spp=1, seed_variant=0, shard_index=0, shard_count=1):
        """IntegratorSinglePlane's gather (plane_single.rs:436-611) through rl_render_plane_single: (image HxWx3 f32, stats dict).  stats: nodes_entered /
        planes_intersected / planes_visible = reserved[0..2], shadow_rays = planes_intersected, ms_other = the gather kernel."""
        return self._render_gather(lib().rl_render_plane_single, planes.h, seeds, spp, seed_variant, shard_index, shard_count,
                                   ("nodes_entered", "planes_intersected", "planes_visible"))

    def render_plane_uncorrelated(self, seeds, nb_primitive=128, strategy="average", spp=1, seed_variant=0, shard_index=0, shard_count=1):
        """IntegratorSinglePlaneUncorrelated behind its block seeds (uncorrelated_plane_single.rs:86-316) through rl_render_plane_uncorrelated: (image HxWx3 f32,
        stats dict).  stats: redraws / planes_intersected / planes_visible = reserved[0..2], shadow_rays = planes_intersected, rng_draws = camera_samples * D +
        2 * redraws, ms_other = the kernel."""
        img, st = self._image_call(seeds, lambda sp, n, out, st: lib().rl_render_plane_uncorrelated(self.h, nb_primitive, plane_strategy(strategy), spp, seed_variant,
                                                                                                    shard_index, shard_count, sp, n, out, st))
        d = st.as_dict()
        d.update((name, int(st.reserved[k])) for k, name in enumerate(("redraws", "planes_intersected", "planes_visible")))
        return img, d

    def render_point_normal(self, seeds, strategy="tr_ex", spp=1, use_aa=True, stream_mode=STREAM_REFERENCE_ORDER, seed_variant=0, shard_index=0, shard_count=1):
        """IntegratorPointNormal behind its block seeds (point_normal.rs:2584-2633) through rl_render_point_normal: (image HxWx3 f32, stats dict).  stats:
        camera_samples, rng_draws, extension_rays = camera rays + phase rays, shadow_rays = visibility rays, vertices = samples that had a distance sampler;
        ms_prepass = the chain pass of a data-dependent strategy in reference order, ms_other = k_pn_pixel."""
        return self._render_pn(PointNormalParams(), lib().rl_point_normal_params_default, lib().rl_render_point_normal, seeds, strategy, spp, use_aa, stream_mode,
                               seed_variant, shard_index, shard_count)

    def render_point_normal_mis(self, seeds, strategy="tr_ex", spp=1, use_aa=True, stream_mode=STREAM_REFERENCE_ORDER, seed_variant=0, shard_index=0, shard_count=1):
        """IntegratorPointNormal with use_mis behind its block seeds (point_normal.rs:2605-2612) through rl_render_point_normal_mis: (image HxWx3 f32, stats
        dict).  Only the distance family of `strategy` matters.  stats: camera_samples, rng_draws, extension_rays = camera rays + phase rays, shadow_rays =
        visibility rays, vertices = samples no defined panic ended (tr, eq) or whose third sampler was Some (clamped, pn); ms_prepass = the chain pass of clamped
        and pn in reference order, ms_other = k_pn_pixel."""
        return self._render_pn(PointNormalMisParams(), lib().rl_point_normal_mis_params_default, lib().rl_render_point_normal_mis, seeds, strategy, spp, use_aa,
                               stream_mode, seed_variant, shard_index, shard_count)

    def render_point_normal_taylor(self, seeds, strategy="eq_tr_taylor_ex", spp=1, use_aa=True, stream_mode=STREAM_REFERENCE_ORDER, seed_variant=0, shard_index=0,
                                   shard_count=1):
        """IntegratorPointNormal's Taylor strategies (PN_TAYLOR_STRATEGIES) behind their block seeds through rl_render_point_normal_taylor: (image HxWx3 f32,
        stats dict).  stats: camera_samples, rng_draws, extension_rays = camera rays, shadow_rays = visibility rays, vertices = samples whose distance sampler
        was Some; ms_prepass = the chain pass in reference order, ms_other = k_pn_pixel.  The two eq phase polynomials in an isotropic medium are
        render_point_normal's eq_ex / eq_clamped_ex; pn_phase_taylor_ex with g = 0 is refused."""
        return self._render_pn(PointNormalTaylorParams(), lib().rl_point_normal_taylor_params_default, lib().rl_render_point_normal_taylor, seeds,
                               pn_taylor_strategy(strategy), spp, use_aa, stream_mode, seed_variant, shard_index, shard_count)

    def render_point_normal_ats(self, seeds, strategy="eq_ex", spp=1, use_aa=True, stream_mode=STREAM_REFERENCE_ORDER, seed_variant=0, shard_index=0, shard_count=1):
        """IntegratorPointNormal over the light tree (a scene built with use_ats) behind its block seeds through rl_render_point_normal_ats: (image HxWx3 f32,
        stats dict).  strategy: one of PN_ATS_STRATEGIES, or (family, value).  The emitter comes from the tree walked with the ray importance (tr_ex: with the
        point importance at the scattering point) and takes three draws; the rest of a sample, the stats and the refusals are render_point_normal's and
        render_point_normal_taylor's.  A scene without the tree, or with an emitter that is no surface, is refused."""
        family, value = pn_ats_strategy(strategy)
        return self._render_pn(PointNormalAtsParams(), lib().rl_point_normal_ats_params_default, lib().rl_render_point_normal_ats, seeds, value, spp, use_aa,
                               stream_mode, seed_variant, shard_index, shard_count, family=family)

    def _render_pn(self, p, defaults, render, seeds, strategy, spp, use_aa, stream_mode, seed_variant, shard_index, shard_count, family=None):
        """render_point_normal, render_point_normal_mis, render_point_normal_taylor and render_point_normal_ats (which hand their strategy's value; the last also its family): the params struct `p` filled by `defaults` and the arguments, one call of `render`."""
        defaults(C.byref(p))
        if family is not None:
            p.family = family
        p.spp, p.strategy, p.use_aa, p.stream_mode, p.seed_variant = spp, pn_strategy(strategy), int(bool(use_aa)), stream_mode, seed_variant
        p.shard_index, p.shard_count = shard_index, shard_count
        img, st = self._image_call(seeds, lambda sp, n, out, st: render(self.h, C.byref(p), sp, n, out, st))
        return img, st.as_dict()

    def trace(self, origins, directions):
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        n = o.shape[0]
        t = np.zeros(n, np.float32); u = np.zeros(n, np.float32); v = np.zeros(n, np.float32)
        m = np.zeros(n, np.int32); tr = np.zeros(n, np.int32)
        _check(lib().rl_trace_batch(self.h, n, abi.fptr(o), abi.fptr(d), abi.fptr(t), abi.fptr(u), abi.fptr(v),
                                    m.ctypes.data_as(C.POINTER(C.c_int32)), tr.ctypes.data_as(C.POINTER(C.c_int32))))
        return t, u, v, m, tr

    def trace_fast(self, origins, directions):
        """Test hook: closest hits through the tolerance build's traversal of a streaming scene (quantised BVH4): (t, mesh, tri, node trips per ray)."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        n = o.shape[0]
        t = np.zeros(n, np.float32); m = np.zeros(n, np.int32); tr = np.zeros(n, np.int32); st = np.zeros(n, np.int32)
        i32p = C.POINTER(C.c_int32)
        fn = lib().rl_debug_trace_batch_fast
        fn.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), i32p, i32p, i32p]
        _check(fn(self.h, n, abi.fptr(o), abi.fptr(d), abi.fptr(t), m.ctypes.data_as(i32p), tr.ctypes.data_as(i32p), st.ctypes.data_as(i32p)))
        return t, m, tr, st

    def trace_two_level(self, origins, directions, segment_lengths=None):
        """Test hook: rl_trace_batch through the two-level node records (trace.hip.h: traverse2): (t, u, v, mesh, tri, node trips per ray); with `segment_lengths`
        the any-hit form: (found, node trips per ray)."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        n = o.shape[0]
        any_hit = segment_lengths is not None
        t = np.ascontiguousarray(segment_lengths, dtype=np.float32).copy() if any_hit else np.zeros(n, np.float32)
        u = np.zeros(n, np.float32); v = np.zeros(n, np.float32)
        m = np.zeros(n, np.int32); tr = np.zeros(n, np.int32); st = np.zeros(n, np.int32)
        i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        fn = lib().rl_debug_trace_batch_two_level
        fn.argtypes = [C.c_void_p, C.c_size_t, f32p, f32p, f32p, f32p, f32p, i32p, i32p, i32p, C.c_int]
        _check(fn(self.h, n, abi.fptr(o), abi.fptr(d), abi.fptr(t), abi.fptr(u), abi.fptr(v), m.ctypes.data_as(i32p), tr.ctypes.data_as(i32p), st.ctypes.data_as(i32p), int(any_hit)))
        return (t != 0.0, st) if any_hit else (t, u, v, m, tr, st)

    def visible(self, p0, p1):
        a = np.ascontiguousarray(p0, dtype=np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(p1, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(a.shape[0], np.uint8)
        _check(lib().rl_visible_batch(self.h, a.shape[0], abi.fptr(a), abi.fptr(b), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def visible_lds(self, p0, p1, packed, capacity=0):
        """Test hook: `visible` on a scene staged in LDS, through the per-lane any-hit loop (packed = False) or the wave's packed form (trace.hip.h: occluded_packed)
        with option shadow_pack_capacity = capacity."""
        a = np.ascontiguousarray(p0, dtype=np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(p1, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(a.shape[0], np.uint8)
        fn = lib().rl_debug_visible_batch_lds
        fn.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_uint8)]
        _check(fn(self.h, a.shape[0], abi.fptr(a), abi.fptr(b), int(bool(packed)), int(capacity), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def debug_sizes(self):
        a, b = C.c_uint64(), C.c_uint64()
        d = C.c_uint32()
        l = C.c_int()
        _check(lib().rl_debug_bvh_sizes(self.h, C.byref(a), C.byref(b), C.byref(d), C.byref(l)))
        return {"ref_nodes": a.value, "prims": b.value, "stack_depth": d.value, "lds_scene": bool(l.value)}


class MultiContext(_ImageCalls):
    """N device contexts of one node + an RCCL communicator clique in ONE process (rl_multi_*): shard renders on one host thread
    per GPU, a single ncclReduce over xGMI, one download from the root."""

    def __init__(self, scene: Scene, n_shards: int, devices=None):
        self.scene = scene
        h = C.c_void_p()
        dv = None if devices is None else (C.c_int * n_shards)(*devices)
        _check(lib().rl_multi_create(scene.h, dv, n_shards, C.byref(h)))
        self.h = h
        self.width, self.height = scene.size

    def info(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        _check(lib().rl_multi_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"shards": a.value, "comm_ranks": b.value, "rccl_version": c.value}

    def describe(self) -> dict:
        """rl_multi_describe: devices, peer access matrix, how the framebuffers are merged, per-shard kernel ms of the last render."""
        import json

        buf = C.create_string_buffer(1 << 16)
        _check(lib().rl_multi_describe(self.h, buf, len(buf)))
        return json.loads(buf.value.decode())

    def shard_stats(self, shard: int):
        dev, st = C.c_int(), abi.RenderStats()
        _check(lib().rl_multi_shard_stats(self.h, shard, C.byref(dev), C.byref(st)))
        return dev.value, st.as_dict()

    def render(self, seeds: np.ndarray, params: abi.PathParams):
        img, st = self._image_call(seeds, lambda sp, n, out, st: lib().rl_multi_render_path(self.h, C.byref(params), sp, n, out, st))
        return img, st.as_dict()

    def close(self):
        if getattr(self, "h", None):
            lib().rl_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stratified_draws(pixel_seeds, spp: int, pattern, seed_variant: int = 0, device: int = 0) -> np.ndarray:
    """Test hook (rl_debug_stratified_draws): the device sampler of STREAM_STRATIFIED.  Pixel p, whose per-sample-mode seed is pixel_seeds[p], walks its
    spp samples as the renderers do; each sample makes the calls of `pattern` (1 = next(), 2 = next2d()).  Returns float32 [n_pixels, spp, n_out]:
    the values in the order drawn (a next2d() gives two), n_out = sum(pattern)."""
    L = lib()
    fn = L.rl_debug_stratified_draws
    fn.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_uint64), C.c_uint32, C.c_int, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_float)]
    seeds = np.ascontiguousarray(pixel_seeds, dtype=np.uint64).reshape(-1)
    pat = np.ascontiguousarray(pattern, dtype=np.int32).reshape(-1)
    out = np.zeros((seeds.shape[0], spp, int(pat.sum())), dtype=np.float32)
    _check(fn(device, seeds.shape[0], abi.u64ptr(seeds), spp, seed_variant, pat.shape[0], pat.ctypes.data_as(C.POINTER(C.c_int32)), abi.fptr(out)))
    return out


class _Integrator:
    """What the integrator classes share: the device, the execution options of every context they create (Context.set_option; none changes an image), the
    stats of the last render and the context of the last scene (the BVH is built once per scene, like BVHAccel::new in IntegratorType::compute)."""

    def __init__(self, device=0, options=None):
        self.device = device
        self.options = dict(options or {})
        self.last_stats = None
        self._ctx = None

    def _new_context(self, scene: Scene) -> "Context":
        c = Context(scene, self.device)
        for k, v in self.options.items():
            c.set_option(k, v)
        return c

    def _context(self, scene: Scene) -> "Context":
        """The context of `scene`: the last one while the scene stays, else a new one."""
        if self._ctx is None or self._ctx.scene is not scene:
            self._ctx = self._new_context(scene)
        return self._ctx


class IntegratorPathTracing(_Integrator):
    """struct IntegratorPathTracing (src/integrators/explicit/path.rs:14-20) + Integrator::compute."""

    def __init__(self, min_depth=0, max_depth=None, rr_depth=0, strategy=STRATEGY_ALL, single_scattering=False,
                 stream_mode=STREAM_REFERENCE_ORDER, device=0, numerics=NUMERICS_EXACT, frames_in_flight=1, options=None):
        """stream_mode: the plugin's default is rustlight's own per-block stream order (seed-for-seed the reference's image);
        STREAM_PER_SAMPLE is the opt-in throughput decomposition, STREAM_STRATIFIED the stratified sampler on it.  frames_in_flight (MI355X-specific, not in the reference): how many
        independent frames `compute_frames` — and the progressive wrappers through it — keep on the GPU at once (one device context and
        one host thread each; the images are those of one frame after the other)."""
        self.min_depth, self.max_depth, self.rr_depth = min_depth, max_depth, rr_depth
        self.strategy, self.single_scattering = strategy, single_scattering
        super().__init__(device, options)
        self.stream_mode, self.numerics = stream_mode, numerics
        self.frames_in_flight = max(1, int(frames_in_flight))
        self._extra = []

    def compute(self, sampler: IndependentSampler, scene: Scene, nb_samples: int = 1):
        """IntegratorType::compute (integrators/mod.rs:274-338): BVH build (untimed) then the render."""
        ctx = self._context(scene)
        w, h = scene.size
        seeds = sampler.block_seeds(w, h)
        p = path_params(nb_samples, self.min_depth, self.max_depth, self.rr_depth, self.strategy, self.single_scattering,
                        self.stream_mode, sampler.variant, numerics=self.numerics)
        img, self.last_stats = ctx.render(seeds, p)
        return img

    def compute_frames(self, sampler: IndependentSampler, scene: Scene, nb_samples: int, n_frames: int):
        """`n_frames` consecutive `compute` calls — the block seeds of every frame are drawn from the master sampler in call order, exactly
        as that many sequential calls would draw them — with up to `frames_in_flight` of them on the GPU at once.  A frame's render is a
        chain of dependent launches that leaves much of the chip idle at its tail (reference-order streams: the chain pass ends with its
        slowest wave); another context's frame fills it.  Returns the images in frame order."""
        before = self._ctx
        if self._context(scene) is not before:
            self._extra = []
        k = min(self.frames_in_flight, max(1, n_frames))
        while len(self._extra) < k - 1:
            self._extra.append(self._new_context(scene))
        w, h = scene.size
        jobs = [(sampler.block_seeds(w, h),
                 path_params(nb_samples, self.min_depth, self.max_depth, self.rr_depth, self.strategy, self.single_scattering,
                             self.stream_mode, sampler.variant, numerics=self.numerics)) for _ in range(n_frames)]
        out = render_in_flight([self._ctx] + self._extra[:k - 1], jobs)
        if out:
            self.last_stats = out[-1][1]
        return [img for img, _ in out]


class IntegratorLightTracing(_Integrator):
    """struct IntegratorLightTracing (src/integrators/explicit/light.rs:7-13) + Integrator::compute: light paths splatted through the camera, on the
    per-sample streams (rl_render_light).  strategy: LIGHT_ALL / LIGHT_SURFACE / LIGHT_VOLUME (render_surface / render_volume)."""

    def __init__(self, min_depth=0, max_depth=None, rr_depth=0, strategy=LIGHT_ALL, device=0, options=None):
        super().__init__(device, options)
        self.min_depth, self.max_depth, self.rr_depth, self.strategy = min_depth, max_depth, rr_depth, strategy

    def compute(self, sampler: IndependentSampler, scene: Scene, nb_samples: int = 1):
        """The block seeds are drawn from the master sampler as IntegratorPathTracing.compute draws them."""
        ctx = self._context(scene)
        w, h = scene.size
        seeds = sampler.block_seeds(w, h)
        img, self.last_stats = ctx.render_light(seeds, nb_samples, self.min_depth, self.max_depth, self.rr_depth, self.strategy, sampler.variant)
        return img


class _DeviceHandle:
    """A handle a Context made (kept alive with it), destroyed through the library function `_destroy` names."""
    _destroy = None

    def __init__(self, h, ctx: "Context"):
        self.h, self.ctx = h, ctx

    def close(self):
        if getattr(self, "h", None):
            getattr(lib(), self._destroy)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _tree_arrays(build, n_elements):
    """The two calls of a tree build: build(capacity, n_nodes, boxes, links, order) first asks the node count with no arrays, then fills
    (boxes [n, 6] f32, links [n, 3] u32, order [n_elements] u32)."""
    n = C.c_size_t()
    _check(build(0, C.byref(n), None, None, None))
    boxes, links, order = np.zeros((n.value, 6), np.float32), np.zeros((n.value, 3), np.uint32), np.zeros(n_elements, np.uint32)
    _check(build(n.value, C.byref(n), abi.fptr(boxes), abi.u32ptr(links), abi.u32ptr(order)))
    return boxes, links, order


class _MapIntegrator(_Integrator):
    """compute of the integrators that gather a map of light-pass records: _generate(ctx, sampler) -> (set, stats), _build(ctx, set) -> map, the block seeds
    from the sampler the generation leaves, _render(ctx, map, seeds, nb_samples, seed_variant) -> (image, stats); map and set are closed, in that order, on
    every path."""

    def compute(self, sampler: IndependentSampler, scene: Scene, nb_samples: int = 1):
        ctx = self._context(scene)
        records, self.last_generation_stats = self._generate(ctx, sampler)
        built = None
        try:
            built = self._build(ctx, records)
            w, h = scene.size
            seeds = sampler.block_seeds(w, h)
            img, self.last_stats = self._render(ctx, built, seeds, nb_samples, sampler.variant)
        finally:
            if built is not None:
                built.close()
            records.close()
        return img


class VplSet(_DeviceHandle):
    """rl_vpl_set: the VPLs of one generation, on the device of the context that made them (kept alive with it)."""
    _destroy = "rl_vpl_destroy"

    def info(self):
        """(VPLs stored, light paths shot)."""
        n, p = C.c_uint64(), C.c_uint64()
        _check(lib().rl_vpl_info(self.h, C.byref(n), C.byref(p)))
        return int(n.value), int(p.value)

    def __len__(self):
        return self.info()[0]

    def words(self) -> np.ndarray:
        """The raw records, [n_vpl, VPL_WORDS] u32 (layout: include/rustlight_amd.h, rl_vpl_read)."""
        n = self.info()[0]
        w = np.zeros((n, VPL_WORDS), np.uint32)
        _check(lib().rl_vpl_read(self.h, abi.u32ptr(w), w.size))
        return w

    def records(self) -> np.ndarray:
        """The records as a numpy structured array: kind, mesh, has_uv, pos, radiance, dir (wi / d_in / n), uv, frame (3 x 3 rows x, y, z)."""
        return self.words().view(VPL_RECORD_DTYPE).reshape(-1)


VPL_RECORD_DTYPE = np.dtype([("kind", "<u4"), ("mesh", "<u4"), ("has_uv", "<u4"), ("pad", "<u4"), ("pos", "<f4", 3), ("radiance", "<f4", 3),
                             ("dir", "<f4", 3), ("uv", "<f4", 2), ("frame", "<f4", (3, 3))])
assert VPL_RECORD_DTYPE.itemsize == 4 * VPL_WORDS


class PhotonMap(_DeviceHandle):
    """rl_photon_map: photon tree and photons of one generation, on the device of the context that made them (kept alive with it)."""
    _destroy = "rl_photon_map_destroy"

    def __init__(self, h, ctx: Context):
        super().__init__(h, ctx)
        self.ms_build = None        # Context.photon_map: wall clock of the build call, ms
        self.ms_kernels = None      # the device build's kernel time, ms

    def read(self):
        """rl_photon_map_read: (boxes [n, 6] f32, links [n, 3] u32 = skip, first, count, photons [n_photons, 9] f32 = pos, radiance, d_in in leaf order)."""
        n_photons, n_nodes, _, _ = self.info()
        boxes, links, photons = np.zeros((n_nodes, 6), np.float32), np.zeros((n_nodes, 3), np.uint32), np.zeros((n_photons, 9), np.float32)
        _check(lib().rl_photon_map_read(self.h, n_nodes, abi.fptr(boxes), abi.u32ptr(links), n_photons, abi.fptr(photons)))
        return boxes, links, photons

    def info(self):
        """(photons, tree nodes, light paths shot, radius)."""
        n, m, p, r = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_float()
        _check(lib().rl_photon_map_info(self.h, C.byref(n), C.byref(m), C.byref(p), C.byref(r)))
        return int(n.value), int(m.value), int(p.value), float(r.value)


def photon_tree_build(words, radius):
    """rl_photon_tree_build, host only: (boxes [n, 6] f32, links [n, 3] u32 = skip, first, count, order [n_photons] u32) of the photon tree over records
    `words` ([n_photons, VPL_WORDS] u32), nodes in the order the gather visits them."""
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, VPL_WORDS)
    return _tree_arrays(lambda *out: lib().rl_photon_tree_build(abi.u32ptr(w), w.shape[0], radius, *out), w.shape[0])


class IntegratorVolPrimitives(_MapIntegrator):
    """struct IntegratorVolPrimitives { nb_primitive, max_depth, rr_depth, primitives } (src/integrators/explicit/vol_primitives.rs) + Integrator::compute for
    primitives = BRE, seed for seed the reference: the photons from the main sampler, the block seeds from the sampler they leave, the gather on
    reference-order streams.  radius: the reference's constant unless given.  light_streams="per_path": the photons from rl_vpl_generate_paths (one light path
    per lane, each on its own stream): statistically, not seed-for-seed, the same image.  tree_build="device": the photon tree from rl_photon_map_build_device
    (the same tree byte for byte, built on the GPU)."""

    def __init__(self, nb_primitive=128, max_depth=None, rr_depth=0, primitives="bre", radius=PHOTON_RADIUS_DEFAULT, device=0, options=None, light_streams="reference",
                 tree_build="host"):
        if primitives != "bre":
            raise RustlightError(RL_ERR_UNSUPPORTED, f"vol-primitives: {primitives} is not built (bre only)")
        if light_streams not in LIGHT_STREAMS:
            raise ValueError(f"light_streams must be one of {LIGHT_STREAMS}, not {light_streams!r}")
        if tree_build not in TREE_BUILDS:
            raise ValueError(f"tree_build must be one of {TREE_BUILDS}, not {tree_build!r}")
        super().__init__(device, options)
        self.light_streams = light_streams
        self.tree_build = tree_build
        self.nb_primitive, self.max_depth, self.rr_depth, self.radius = nb_primitive, max_depth, rr_depth, radius
        self.last_generation_stats = None

    def _generate(self, ctx, sampler):
        return ctx.vpl_generate(sampler, self.nb_primitive, self.max_depth, self.rr_depth, VPL_VOLUME, self.light_streams)

    def _build(self, ctx, vpls):
        return ctx.photon_map(vpls, self.radius, self.tree_build)

    _render = staticmethod(Context.render_bre)


class _BeamPassIntegrator(_MapIntegrator):
    """IntegratorPhotonBeams, IntegratorVirtualRayLights and IntegratorPhotonPlanes: the same fields, and _MapIntegrator's compute over the three Context
    methods `_calls` names (the beam or plane pass, the map build, the gather)."""
    _calls = None

    def __init__(self, nb_primitive=128, max_depth=None, rr_depth=0, radius=PHOTON_RADIUS_DEFAULT, light_streams="reference", device=0, options=None):
        if light_streams not in LIGHT_STREAMS:
            raise ValueError(f"light_streams must be one of {LIGHT_STREAMS}, not {light_streams!r}")
        super().__init__(device, options)
        self.nb_primitive, self.max_depth, self.rr_depth, self.radius, self.light_streams = nb_primitive, max_depth, rr_depth, radius, light_streams
        self.last_generation_stats = None

    def _generate(self, ctx, sampler):
        return getattr(ctx, self._calls[0])(sampler, self.nb_primitive, self.max_depth, self.rr_depth, self.light_streams)

    def _build(self, ctx, records):
        return getattr(ctx, self._calls[1])(records, self.radius)

    def _render(self, ctx, *args):
        return getattr(ctx, self._calls[2])(*args)


class BeamSet(_DeviceHandle):
    """rl_beam_set: the beams of one beam pass, on the device of the context that made them (kept alive with it)."""
    _destroy = "rl_beam_destroy"

    def info(self):
        """(beams stored, light paths shot)."""
        n, p = C.c_uint64(), C.c_uint64()
        _check(lib().rl_beam_info(self.h, C.byref(n), C.byref(p)))
        return int(n.value), int(p.value)

    def __len__(self):
        return self.info()[0]

    def words(self) -> np.ndarray:
        """The raw records, [n_beams, BEAM_WORDS] u32 (layout: include/rustlight_amd.h, rl_beam_read)."""
        w = np.zeros((self.info()[0], BEAM_WORDS), np.uint32)
        _check(lib().rl_beam_read(self.h, abi.u32ptr(w), w.size))
        return w

    def records(self) -> np.ndarray:
        """The records as a numpy structured array: o, length, d, flags (bit 0 = from_surface), radiance, path."""
        return self.words().view(BEAM_RECORD_DTYPE).reshape(-1)


BEAM_RECORD_DTYPE = np.dtype([("o", "<f4", 3), ("length", "<f4"), ("d", "<f4", 3), ("flags", "<u4"), ("radiance", "<f4", 3), ("path", "<u4")])
assert BEAM_RECORD_DTYPE.itemsize == 4 * BEAM_WORDS


class BeamMap(_DeviceHandle):
    """rl_beam_map: beam tree and sub-beams of one beam pass, on the device of the context that made them (kept alive with it)."""
    _destroy = "rl_beam_map_destroy"

    def info(self):
        """(beams, sub-beams, tree nodes, light paths shot, radius)."""
        n, s_, m, p, r = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_float()
        _check(lib().rl_beam_map_info(self.h, C.byref(n), C.byref(s_), C.byref(m), C.byref(p), C.byref(r)))
        return int(n.value), int(s_.value), int(m.value), int(p.value), float(r.value)

    def read(self):
        """rl_beam_map_read: (boxes [n, 6] f32, links [n, 3] u32 = skip, first, count, beams [n_sub, 12] f32 = o, length | d, 0 | radiance, 0 in leaf order)."""
        _, n_sub, n_nodes, _, _ = self.info()
        boxes, links, beams = np.zeros((n_nodes, 6), np.float32), np.zeros((n_nodes, 3), np.uint32), np.zeros((n_sub, 12), np.float32)
        _check(lib().rl_beam_map_read(self.h, n_nodes, abi.fptr(boxes), abi.u32ptr(links), n_sub, abi.fptr(beams)))
        return boxes, links, beams


def beam_split(words):
    """rl_beam_split, host only: the sub-beams ([n_sub, BEAM_WORDS] u32, in beam order) of beam records `words` ([n, BEAM_WORDS] u32)."""
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, BEAM_WORDS)
    n = C.c_size_t()
    _check(lib().rl_beam_split(abi.u32ptr(w), w.shape[0], 0, C.byref(n), None))
    sub = np.zeros((n.value, BEAM_WORDS), np.uint32)
    _check(lib().rl_beam_split(abi.u32ptr(w), w.shape[0], n.value, C.byref(n), abi.u32ptr(sub)))
    return sub


def beam_tree_build(sub_words, radius):
    """rl_beam_tree_build, host only: photon_tree_build's arrays for the beam tree over sub-beam records ([n_sub, BEAM_WORDS] u32)."""
    w = np.ascontiguousarray(sub_words, dtype=np.uint32).reshape(-1, BEAM_WORDS)
    return _tree_arrays(lambda *out: lib().rl_beam_tree_build(abi.u32ptr(w), w.shape[0], radius, *out), w.shape[0])


class IntegratorPhotonBeams(_BeamPassIntegrator):
    """IntegratorVolPrimitives { nb_primitive, max_depth, rr_depth, primitives: Beams } (src/integrators/explicit/vol_primitives.rs) + Integrator::compute, seed
    for seed the reference: the beams from the main sampler, the split, the beam tree, the block seeds from the sampler the beam pass leaves, the gather on
    reference-order streams.  A class of its own: IntegratorVolPrimitives keeps refusing every primitive but bre.  radius: the reference's constant unless
    given.  light_streams="per_path": the beams from rl_beam_generate_paths: statistically, not seed-for-seed, the same image."""

    _calls = ("beam_generate", "beam_map", "render_beams")


class VrlMap(_DeviceHandle):
    """rl_vrl_map: beam tree and sub-beams of the surface beams, and the VRLs, of one beam pass, on the device of the context that made them (kept alive with it)."""
    _destroy = "rl_vrl_map_destroy"

    def info(self):
        """(surface beams, sub-beams, tree nodes, VRLs, light paths shot, radius, avg)."""
        v = [C.c_uint64() for _ in range(5)]
        r, a = C.c_float(), C.c_float()
        _check(lib().rl_vrl_map_info(self.h, *[C.byref(x) for x in v], C.byref(r), C.byref(a)))
        return tuple(int(x.value) for x in v) + (float(r.value), float(a.value))

    def read(self):
        """rl_vrl_map_read: (boxes [n, 6] f32, links [n, 3] u32 = skip, first, count, beams [n_sub, 12] f32 in leaf order, vrls [n_vrl, 12] f32 = o, length | d, rr
        | radiance, 0 in storing order)."""
        _, n_sub, n_nodes, n_vrl, _, _, _ = self.info()
        boxes, links = np.zeros((n_nodes, 6), np.float32), np.zeros((n_nodes, 3), np.uint32)
        beams, vrls = np.zeros((n_sub, 12), np.float32), np.zeros((n_vrl, 12), np.float32)
        _check(lib().rl_vrl_map_read(self.h, n_nodes, abi.fptr(boxes), abi.u32ptr(links), n_sub, abi.fptr(beams), n_vrl, abi.fptr(vrls)))
        return boxes, links, beams, vrls


class IntegratorVirtualRayLights(_BeamPassIntegrator):
    """IntegratorVolPrimitives { nb_primitive, max_depth, rr_depth, primitives: VRL } (src/integrators/explicit/vol_primitives.rs) + Integrator::compute, seed for
    seed the reference: the beams from the main sampler, the partition, the split and tree of the surface beams, the block seeds from the sampler the beam pass
    leaves, the gather on reference-order streams.  A class of its own: IntegratorVolPrimitives keeps refusing every primitive but bre.  radius: the reference's
    constant unless given.  light_streams="per_path": the beams from rl_beam_generate_paths: statistically, not seed-for-seed, the same image."""

    _calls = ("beam_generate", "vrl_map", "render_vrl")


class PPlaneSet(_DeviceHandle):
    """rl_pplane_set: the planes and surface beams of one plane pass, on the device of the context that made them (kept alive with it)."""
    _destroy = "rl_pplane_destroy"

    def info(self):
        """(planes stored, beams stored, light paths shot)."""
        n, b, p = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().rl_pplane_info(self.h, C.byref(n), C.byref(b), C.byref(p)))
        return int(n.value), int(b.value), int(p.value)

    def __len__(self):
        return self.info()[0]

    def words(self):
        """The raw records: (planes [n_planes, PLANE_WORDS] u32, beams [n_beams, BEAM_WORDS] u32) (layouts: include/rustlight_amd.h, rl_pplane_read)."""
        n, b, _ = self.info()
        pw, bw = np.zeros((n, PLANE_WORDS), np.uint32), np.zeros((b, BEAM_WORDS), np.uint32)
        _check(lib().rl_pplane_read(self.h, abi.u32ptr(pw), pw.size, abi.u32ptr(bw), bw.size))
        return pw, bw

    def records(self):
        """The records as numpy structured arrays: (planes: o, d0, d1, length0, length1, radiance, path, edge; beams: BEAM_RECORD_DTYPE)."""
        pw, bw = self.words()
        return pw.view(PPLANE_RECORD_DTYPE).reshape(-1), bw.view(BEAM_RECORD_DTYPE).reshape(-1)


PPLANE_RECORD_DTYPE = np.dtype([("o", "<f4", 3), ("d0", "<f4", 3), ("d1", "<f4", 3), ("length0", "<f4"), ("length1", "<f4"), ("radiance", "<f4", 3), ("path", "<u4"),
                                ("edge", "<u4"), ("zero", "<u4", 2)])
assert PPLANE_RECORD_DTYPE.itemsize == 4 * PLANE_WORDS


class PPlaneMap(_DeviceHandle):
    """rl_pplane_map: beam tree, sub-beams, plane tree and planes of one plane pass, on the device of the context that made them (kept alive with it)."""
    _destroy = "rl_pplane_map_destroy"

    def info(self):
        """(beams, sub-beams, beam-tree nodes, planes, plane-tree nodes, light paths shot, radius)."""
        v = [C.c_uint64() for _ in range(6)]
        r = C.c_float()
        _check(lib().rl_pplane_map_info(self.h, *[C.byref(x) for x in v], C.byref(r)))
        return tuple(int(x.value) for x in v) + (float(r.value),)

    def read(self, which):
        """rl_pplane_map_read: (boxes [n, 6] f32, links [n, 3] u32 = skip, first, count, elements in leaf order) of which = "beams" ([n_sub, 12] f32 = o, length
        | d, 0 | radiance, 0) or "planes" ([n_planes, 16] f32 = o, length0 | d0, length1 | d1, 0 | radiance, 0)."""
        if which not in ("beams", "planes"):
            raise ValueError(f"which must be 'beams' or 'planes', not {which!r}")
        _, n_sub, n_bn, n_planes, n_pn, _, _ = self.info()
        n_nodes, n_el, width = (n_bn, n_sub, 12) if which == "beams" else (n_pn, n_planes, 16)
        boxes, links, el = np.zeros((n_nodes, 6), np.float32), np.zeros((n_nodes, 3), np.uint32), np.zeros((n_el, width), np.float32)
        _check(lib().rl_pplane_map_read(self.h, 0 if which == "beams" else 1, n_nodes, abi.fptr(boxes), abi.u32ptr(links), n_el, abi.fptr(el)))
        return boxes, links, el


class IntegratorPhotonPlanes(_BeamPassIntegrator):
    """IntegratorVolPrimitives { nb_primitive, max_depth, rr_depth, primitives: Planes } (src/integrators/explicit/vol_primitives.rs) + Integrator::compute, seed
    for seed the reference: surface beams and planes from the main sampler, the split, the two trees, the block seeds from the sampler the plane pass leaves,
    the gather on reference-order streams.  A class of its own: IntegratorVolPrimitives keeps refusing every primitive but bre.  radius: the reference's
    constant unless given.  light_streams="per_path": the records from rl_pplane_generate_paths: statistically, not seed-for-seed, the same image."""

    _calls = ("pplane_generate", "pplane_map", "render_photon_planes")


def plane_strategy(strategy):
    """rl_plane_strategy of a name of PLANE_STRATEGIES (or of its value)."""
    if isinstance(strategy, str):
        if strategy not in PLANE_STRATEGIES:
            raise ValueError(f"{strategy} is not a correct strategy choice (uv, ut, vt, average, discrete_mis, valpha, cmis)")
        return PLANE_STRATEGIES.index(strategy)
    return int(strategy)


class PlaneSet(_DeviceHandle):
    """rl_plane_set: the planes of one rl_plane_generate."""
    _destroy = "rl_plane_destroy"

    def info(self):
        """(planes stored, number_plane_gen, strategy name)."""
        n, g, s = C.c_uint64(), C.c_uint64(), C.c_int()
        _check(lib().rl_plane_info(self.h, C.byref(n), C.byref(g), C.byref(s)))
        return int(n.value), int(g.value), PLANE_STRATEGIES[s.value]

    def __len__(self):
        return self.info()[0]

    def words(self) -> np.ndarray:
        """The raw records, [n_planes, PLANE_WORDS] u32 (layout: include/rustlight_amd.h, rl_plane_read)."""
        w = np.zeros((self.info()[0], PLANE_WORDS), np.uint32)
        _check(lib().rl_plane_read(self.h, abi.u32ptr(w), w.size))
        return w


class PlaneMap(_DeviceHandle):
    """rl_plane_map: plane tree, planes and lights of one generation, on the device of the context that made them (kept alive with it)."""
    _destroy = "rl_plane_map_destroy"

    def __init__(self, h, ctx: Context):
        super().__init__(h, ctx)
        self.ms_build = None        # Context.plane_map: wall clock of the build call, ms
        self.ms_kernels = None      # build="device": HIP-event time of its launches, ms

    def info(self):
        """(planes, tree nodes, number_plane_gen, strategy name)."""
        n, m, g, s = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
        _check(lib().rl_plane_map_info(self.h, C.byref(n), C.byref(m), C.byref(g), C.byref(s)))
        return int(n.value), int(m.value), int(g.value), PLANE_STRATEGIES[s.value]

    def read(self):
        """rl_plane_map_read: (boxes [n, 6] f32, links [n, 3] u32 = skip, first, count, planes [n_planes, 16] f32 in leaf order)."""
        n_planes, n_nodes, _, _ = self.info()
        boxes, links, planes = np.zeros((n_nodes, 6), np.float32), np.zeros((n_nodes, 3), np.uint32), np.zeros((n_planes, 16), np.float32)
        _check(lib().rl_plane_map_read(self.h, n_nodes, abi.fptr(boxes), abi.u32ptr(links), n_planes, abi.fptr(planes)))
        return boxes, links, planes


def plane_tree_build(words):
    """rl_plane_tree_build, host only: (boxes [n, 6] f32, links [n, 3] u32 = skip, first, count, order [n_planes] u32) of the plane tree over records
    `words` ([n_planes, PLANE_WORDS] u32), nodes in the order the gather visits them."""
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, PLANE_WORDS)
    return _tree_arrays(lambda *out: lib().rl_plane_tree_build(abi.u32ptr(w), w.shape[0], *out), w.shape[0])


class IntegratorSinglePlane(_MapIntegrator):
    """struct IntegratorSinglePlane { nb_primitive, strategy } (src/integrators/explicit/plane_single.rs:291-294) + Integrator::compute, seed for seed the
    reference: the planes from the main sampler, the plane tree, the block seeds from the sampler the generation leaves, the gather on reference-order streams.
    generate="lanes" / tree_build="device": the plane pass on one lane per iteration and the tree from device kernels, byte for byte the same planes and map."""

    def __init__(self, nb_primitive=128, strategy="average", device=0, options=None, generate="serial", tree_build="host"):
        super().__init__(device, options)
        if generate not in PLANE_FORMS:
            raise ValueError(f"generate must be one of {PLANE_FORMS}, not {generate!r}")
        if tree_build not in TREE_BUILDS:
            raise ValueError(f"tree_build must be one of {TREE_BUILDS}, not {tree_build!r}")
        self.generate, self.tree_build = generate, tree_build
        self.nb_primitive, self.strategy = nb_primitive, PLANE_STRATEGIES[plane_strategy(strategy)]
        self.last_generation_stats = None

    def _generate(self, ctx, sampler):
        return ctx.plane_generate(sampler, self.nb_primitive, self.strategy, self.generate)

    def _build(self, ctx, planes):
        return ctx.plane_map(planes, self.tree_build)

    _render = staticmethod(Context.render_plane_single)


class IntegratorSinglePlaneUncorrelated(_Integrator):
    """struct IntegratorSinglePlaneUncorrelated { nb_primitive, strategy } (src/integrators/explicit/uncorrelated_plane_single.rs:8-11) + Integrator::compute, seed
    for seed the reference: the block seeds straight from the main sampler (:83), then every camera sample makes and gathers its own planes."""

    def __init__(self, nb_primitive=128, strategy="average", device=0, options=None):
        super().__init__(device, options)
        self.nb_primitive, self.strategy = nb_primitive, PLANE_STRATEGIES[plane_strategy(strategy)]

    def compute(self, sampler: IndependentSampler, scene: Scene, nb_samples: int = 1):
        ctx = self._context(scene)
        w, h = scene.size
        seeds = sampler.block_seeds(w, h)
        img, self.last_stats = ctx.render_plane_uncorrelated(seeds, self.nb_primitive, self.strategy, nb_samples, sampler.variant)
        return img


def pn_strategy(strategy):
    """rl_pn_strategy of a name of PN_STRATEGIES (or of its value)."""
    if isinstance(strategy, str):
        if strategy not in PN_STRATEGIES:
            raise ValueError(f"invalid strategy: {strategy} ({', '.join(PN_STRATEGIES)})")
        return PN_STRATEGIES.index(strategy)
    return int(strategy)


def pn_ats_strategy(strategy):
    """(rl_pn_ats_family, the strategy's value within it) of a name of PN_ATS_STRATEGIES, or of such a pair."""
    if isinstance(strategy, str):
        if strategy not in PN_ATS_STRATEGIES:
            raise ValueError(f"invalid strategy: {strategy} ({', '.join(PN_ATS_STRATEGIES)})")
        return (0, PN_STRATEGIES.index(strategy)) if strategy in PN_STRATEGIES else (1, PN_TAYLOR_STRATEGIES.index(strategy))
    family, value = strategy
    return int(family), int(value)


def pn_taylor_strategy(strategy):
    """rl_pn_taylor_strategy of a name of PN_TAYLOR_STRATEGIES (or of its value)."""
    if isinstance(strategy, str):
        if strategy not in PN_TAYLOR_STRATEGIES:
            raise ValueError(f"invalid strategy: {strategy} ({', '.join(PN_TAYLOR_STRATEGIES)})")
        return PN_TAYLOR_STRATEGIES.index(strategy)
    return int(strategy)


class IntegratorPointNormal(_Integrator):
    """struct IntegratorPointNormal { strategy, use_mis, warps, warps_strategy, splitting, use_aa } (src/integrators/explicit/point_normal.rs:1172-1179) +
    Integrator::compute -> compute_mc, seed for seed the reference: the block seeds straight from the main sampler, then rl_render_point_normal.  The seven
    plain strategies of PN_STRATEGIES; MIS, splitting, the warps and the flavoured strategies are not built."""

    def __init__(self, strategy="tr_ex", use_aa=True, stream_mode=STREAM_REFERENCE_ORDER, device=0, options=None):
        super().__init__(device, options)
        self.strategy, self.use_aa, self.stream_mode = PN_STRATEGIES[pn_strategy(strategy)], use_aa, stream_mode

    def compute(self, sampler: IndependentSampler, scene: Scene, nb_samples: int = 1):
        ctx = self._context(scene)
        w, h = scene.size
        seeds = sampler.block_seeds(w, h)
        img, self.last_stats = ctx.render_point_normal(seeds, self.strategy, nb_samples, self.use_aa, self.stream_mode, sampler.variant)
        return img


class IntegratorPointNormalMis(_Integrator):
    """IntegratorPointNormal with use_mis = true (src/integrators/explicit/point_normal.rs:1172-1179, 2605-2612) + Integrator::compute -> compute_mc, seed for
    seed the reference: the block seeds straight from the main sampler, then rl_render_point_normal_mis.  Only the distance family of the strategy selects the
    estimator (tr, eq, clamped, pn); the two names of a family render the same bytes."""

    def __init__(self, strategy="tr_ex", use_aa=True, stream_mode=STREAM_REFERENCE_ORDER, device=0, options=None):
        super().__init__(device, options)
        self.strategy, self.use_aa, self.stream_mode = PN_STRATEGIES[pn_strategy(strategy)], use_aa, stream_mode

    def compute(self, sampler: IndependentSampler, scene: Scene, nb_samples: int = 1):
        ctx = self._context(scene)
        w, h = scene.size
        seeds = sampler.block_seeds(w, h)
        img, self.last_stats = ctx.render_point_normal_mis(seeds, self.strategy, nb_samples, self.use_aa, self.stream_mode, sampler.variant)
        return img


class IntegratorPointNormalTaylor(_Integrator):
    """IntegratorPointNormal with one of the six Taylor strategies of PN_TAYLOR_STRATEGIES (src/integrators/explicit/point_normal.rs:1276-1290, 1404-1418) +
    Integrator::compute -> compute_mc, seed for seed the reference: the block seeds straight from the main sampler, then rl_render_point_normal_taylor."""

    def __init__(self, strategy="eq_tr_taylor_ex", use_aa=True, stream_mode=STREAM_REFERENCE_ORDER, device=0, options=None):
        super().__init__(device, options)
        self.strategy, self.use_aa, self.stream_mode = PN_TAYLOR_STRATEGIES[pn_taylor_strategy(strategy)], use_aa, stream_mode

    def compute(self, sampler: IndependentSampler, scene: Scene, nb_samples: int = 1):
        ctx = self._context(scene)
        w, h = scene.size
        seeds = sampler.block_seeds(w, h)
        img, self.last_stats = ctx.render_point_normal_taylor(seeds, self.strategy, nb_samples, self.use_aa, self.stream_mode, sampler.variant)
        return img


class IntegratorPointNormalAts(_Integrator):
    """IntegratorPointNormal over the light tree with one of the names of PN_ATS_STRATEGIES (fix_random_sample_emitter's ATS arm,
    src/integrators/explicit/point_normal.rs:1217-1228, and compute_single_tr's, :2237-2243) + Integrator::compute -> compute_mc, seed for seed the reference:
    the block seeds straight from the main sampler, then rl_render_point_normal_ats.  The scene's emitters are built with the tree (use_ats)."""

    def __init__(self, strategy="eq_ex", use_aa=True, stream_mode=STREAM_REFERENCE_ORDER, device=0, options=None):
        super().__init__(device, options)
        pn_ats_strategy(strategy)
        self.strategy, self.use_aa, self.stream_mode = strategy, use_aa, stream_mode

    def compute(self, sampler: IndependentSampler, scene: Scene, nb_samples: int = 1):
        ctx = self._context(scene)
        w, h = scene.size
        seeds = sampler.block_seeds(w, h)
        img, self.last_stats = ctx.render_point_normal_ats(seeds, self.strategy, nb_samples, self.use_aa, self.stream_mode, sampler.variant)
        return img


class IntegratorVPL(_Integrator):
    """struct IntegratorVPL (src/integrators/explicit/vpl.rs:16-23) + Integrator::compute, seed for seed the reference: the VPLs from the main sampler, the
    block seeds from the sampler they leave, the gather on reference-order streams.  clamping_factor is not a field: the reference never reads it.  light_streams="per_path": the VPLs from
    rl_vpl_generate_paths (one light path per lane, each on its own stream): statistically, not seed-for-seed, the same image."""

    def __init__(self, nb_vpl=128, max_depth=None, rr_depth=0, option_vpl=VPL_ALL, option_lt=VPL_ALL, device=0, options=None, light_streams="reference"):
        if light_streams not in LIGHT_STREAMS:
            raise ValueError(f"light_streams must be one of {LIGHT_STREAMS}, not {light_streams!r}")
        super().__init__(device, options)
        self.light_streams = light_streams
        self.nb_vpl, self.max_depth, self.rr_depth = nb_vpl, max_depth, rr_depth
        self.option_vpl, self.option_lt = option_vpl, option_lt
        self.last_generation_stats = None

    def compute(self, sampler: IndependentSampler, scene: Scene, nb_samples: int = 1):
        ctx = self._context(scene)
        vpls, self.last_generation_stats = ctx.vpl_generate(sampler, self.nb_vpl, self.max_depth, self.rr_depth, self.option_vpl, self.light_streams)
        try:
            w, h = scene.size
            seeds = sampler.block_seeds(w, h)
            img, self.last_stats = ctx.render_vpl(vpls, seeds, nb_samples, self.option_lt, sampler.variant)
        finally:
            vpls.close()
        return img


def render_frames(contexts, seeds_list, params: abi.PathParams):
    """rl_render_path_frames: the frames of `seeds_list` (block seeds per frame) with the same parameters, frame f on contexts[f % len(contexts)] — the library's own
    threads.  Returns ([image, ...], [stats dict, ...]) in frame order."""
    n = len(seeds_list)
    w, h = contexts[0].width, contexts[0].height
    seeds = [np.ascontiguousarray(s, dtype=np.uint64) for s in seeds_list]
    imgs = [np.zeros((h, w, 3), dtype=np.float32) for _ in range(n)]
    vp, u64p, fp = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_float)
    c_ctx = (vp * len(contexts))(*[c.h.value for c in contexts])
    c_seeds = (u64p * max(n, 1))(*[abi.u64ptr(s) for s in seeds])
    c_out = (fp * max(n, 1))(*[abi.fptr(i) for i in imgs])
    st = (abi.RenderStats * max(n, 1))()
    _check(lib().rl_render_path_frames(c_ctx, len(contexts), C.byref(params), c_seeds, seeds[0].shape[0] if n else 0, n, c_out, st))
    return imgs, [st[f].as_dict() for f in range(n)]


def render_in_flight(contexts, jobs):
    """Render `jobs` = [(block seeds, path params), ...] on `contexts` (same scene, any devices), job j on context j % len(contexts), one host
    thread per context (rl_render_path is synchronous; contexts own their streams and share nothing mutable, and ctypes releases the GIL
    for the call).  Returns [(image, stats), ...] in job order; the first error is re-raised after every thread has stopped."""
    import threading
    k = max(1, min(len(contexts), len(jobs)))
    out = [None] * len(jobs)
    errors = []

    def work(c):
        try:
            for j in range(c, len(jobs), k):
                if errors:
                    return
                out[j] = contexts[c].render(*jobs[j])
        except Exception as e:      # noqa: BLE001 — handed to the caller below
            errors.append(e)

    if k == 1:
        work(0)
    else:
        threads = [threading.Thread(target=work, args=(c,)) for c in range(k)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    if errors:
        raise errors[0]
    return out


def _load_with(fn_name: str, path: str) -> np.ndarray:
    w, h = C.c_uint32(), C.c_uint32()
    fn = getattr(lib(), fn_name)
    fn.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_size_t]
    _check(fn(path.encode(), C.byref(w), C.byref(h), None, 0))
    out = np.zeros((h.value, w.value, 3), np.float32)
    _check(fn(path.encode(), C.byref(w), C.byref(h), abi.fptr(out), out.size))
    return out


def load_pfm(path: str) -> np.ndarray:
    """Bitmap::read_pfm (src/structure.rs:563-607) -> H x W x 3 float32, top row first."""
    return _load_with("rl_load_pfm", path)


def load_image(path: str) -> np.ndarray:
    """Bitmap::read (src/structure.rs:670-683): .pfm / .png -> H x W x 3 float32."""
    return _load_with("rl_load_image", path)


def save_pfm(path: str, img: np.ndarray):
    a = np.ascontiguousarray(img, dtype=np.float32)
    _check(lib().rl_save_pfm(path.encode(), abi.fptr(a), a.shape[1], a.shape[0]))


def save_image(path: str, img: np.ndarray):
    """Bitmap::save: .pfm | .png | .exr by extension (src/structure.rs:528-545)."""
    a = np.ascontiguousarray(img, dtype=np.float32)
    _check(lib().rl_save_image(path.encode(), abi.fptr(a), a.shape[1], a.shape[0]))


class IntegratorAverage:
    """IntegratorAverage { time_out, integrator, dump_all } (src/integrators/avg.rs:5-131): re-runs the inner integrator with
    the same, advancing master sampler, keeps the running average, dumps `<base>_<iter>.<ext>` and `<base>_time.csv`."""

    def __init__(self, integrator, time_out=None, dump_all=True, max_iterations=None):
        self.integrator, self.time_out, self.dump_all, self.max_iterations = integrator, time_out, dump_all, max_iterations
        self.iterations = 0

    def compute(self, sampler, scene, nb_samples=1, output_img_path="out.pfm"):
        import time
        if not self.dump_all and self.time_out is None and self.max_iterations is None:
            raise ValueError("Impossible to have infinite approach and not dumping all images")
        base, ext = os.path.splitext(output_img_path)
        csv = open(base + "_time.csv", "w") if self.dump_all else None
        bitmap, iteration, elapsed = None, 1, 0.0
        # frames in flight (an inner integrator that has `frames_in_flight` > 1): the passes are rendered a batch at a time and folded in pass order, each
        # charged its share of the batch's time; with a time-out the passes of the last batch beyond it are dropped (their seeds are drawn: the next
        # call of the same sampler goes on after them)
        batch = max(1, getattr(self.integrator, "frames_in_flight", 1)) if hasattr(self.integrator, "compute_frames") else 1
        pending = []
        while True:
            t0 = time.perf_counter()
            if batch > 1:
                if not pending:
                    n = batch if self.max_iterations is None else min(batch, self.max_iterations - iteration + 1)
                    pending = self.integrator.compute_frames(sampler, scene, nb_samples, n)
                    share = (time.perf_counter() - t0) / len(pending)
                new = pending.pop(0)
                t0 = time.perf_counter() - share
            else:
                new = self.integrator.compute(sampler, scene, nb_samples)
            if iteration == 1:
                bitmap = new
            else:   # bitmap.scale(iteration); accumulate_bitmap; scale(1 / (iteration + 1))   (avg.rs:59-61, sic)
                bitmap = ((bitmap * np.float32(iteration)) + new) * (np.float32(1.0) / np.float32(iteration + 1))
            elapsed += time.perf_counter() - t0
            if self.dump_all:
                save_image(f"{base}_{iteration}{ext}", bitmap)
                csv.write(f"{int(elapsed)}.{int((elapsed % 1) * 1000)},\n")
            self.iterations = iteration
            if (self.time_out is not None and int(elapsed) >= self.time_out) or (self.max_iterations is not None and iteration >= self.max_iterations):
                break
            iteration += 1
        if csv:
            csv.close()
        return bitmap


class IntegratorEqualTime:
    """IntegratorEqualTime { target_time_ms, integrator } (src/integrators/equal_time.rs:4-66)."""

    def __init__(self, integrator, target_time_ms):
        self.integrator, self.target_time_ms = integrator, target_time_ms
        self.iterations = 0

    def compute(self, sampler, scene, nb_samples=1):
        import time
        bitmap, iteration, elapsed = None, 1, 0.0
        batch = max(1, getattr(self.integrator, "frames_in_flight", 1)) if hasattr(self.integrator, "compute_frames") else 1      # frames in flight: as in IntegratorAverage
        pending = []
        while True:
            t0 = time.perf_counter()
            if batch > 1:
                if not pending:
                    pending = self.integrator.compute_frames(sampler, scene, nb_samples, batch)
                    share = (time.perf_counter() - t0) / len(pending)
                new = pending.pop(0)
                t0 = time.perf_counter() - share
            else:
                new = self.integrator.compute(sampler, scene, nb_samples)
            bitmap = new if iteration == 1 else bitmap + new
            elapsed += time.perf_counter() - t0
            if elapsed * 1000.0 >= self.target_time_ms:
                break
            iteration += 1
        self.iterations = iteration
        return bitmap * (np.float32(1.0) / np.float32(iteration))


def numerics_probe(a: np.ndarray, b: np.ndarray, device: int = 0) -> np.ndarray:
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    out = np.zeros((10, a.shape[0]), np.float32)
    _check(lib().rl_debug_numerics(device, a.shape[0], abi.fptr(a), abi.fptr(b), abi.fptr(out)))
    return out


# rl_math_fn / rl_math_where (csrc/kernels/wavefront.h); codes 0 ... 7 are orc_math_batch's
MATH_FN = {"sinf": 0, "cosf": 1, "expf": 2, "logf": 3, "powf": 4, "acosf": 5, "atan2f": 6, "asinf": 7, "sqrt_rn": 8, "div_rn": 9, "mul_add": 10}
MATH_ON_DEVICE, MATH_ON_HOST = 0, 1
MATH_HOST_FNS = ("sinf", "cosf", "acosf", "atan2f", "asinf")      # what detmath_shared.h holds: the host arm knows nothing else


def math_sweep(fn: str, first_bits: int, stride: int, n: int, b=None, swap: bool = False, period: int = 0, where: int = MATH_ON_DEVICE, device: int = 0) -> np.ndarray:
    """Test hook (rl_debug_math_sweep): out[i] = fn(g_i, b_i), or fn(b_i, g_i) with swap, where g_i is the f32 whose bits are first_bits + (i mod period) * stride
    (mod 2^32; period 0 = no wrap) and b is None (unary), one number or an array of n.  where = MATH_ON_HOST runs the host compiler's copy of
    detmath_shared.h (MATH_HOST_FNS) and touches no GPU."""
    out = np.empty(n, np.float32)
    if b is None:
        bp, nb = None, 0
    else:
        b = np.ascontiguousarray(np.atleast_1d(b), np.float32)
        assert b.shape in ((1,), (n,)), (b.shape, n)
        bp, nb = abi.fptr(b), b.shape[0]
    _check(lib().rl_debug_math_sweep(device, where, MATH_FN[fn], first_bits & 0xffffffff, stride & 0xffffffff, period, n, bp, nb, int(swap), abi.fptr(out)))
    return out
