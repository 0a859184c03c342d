"""Scene and context builders that several test files share (a plain module: `from tests.scene_helpers import ...`)."""
import os

import numpy as np

from rustlight_amd import api, scenes


def context(sd, streaming=False):
    """streaming: the BVH streamed from L2 / HBM instead of staged in LDS (RL_FORCE_STREAMING is read when the context is created)."""
    old = os.environ.pop("RL_FORCE_STREAMING", None)
    if streaming:
        os.environ["RL_FORCE_STREAMING"] = "1"
    try:
        return api.Context(api.Scene(sd), 0)
    finally:
        os.environ.pop("RL_FORCE_STREAMING", None)
        if old is not None:
            os.environ["RL_FORCE_STREAMING"] = old


def with_back_triangle(sd):
    # as test_cbox_medium: a triangle behind the camera stretches the root box over the camera, so that medium vertices can reach it
    back = scenes.MeshData("Back", np.asarray([[0.0, 1.0, 8.0], [0.01, 1.0, 8.0], [0.0, 1.01, 8.0]], dtype=np.float32), np.asarray([[0, 1, 2]], dtype=np.uint32),
                           None, None, scenes.matte((0.5, 0.5, 0.5)))
    sd.meshes.insert(0, back)
    return sd


def add_second_light(sd):
    """A second emissive quad on the left wall; its u x v = (0, 0, 1) x (0, -1, 0) = (1, 0, 0) points into the room."""
    quad = [-0.98, 0.8, -0.3, -0.98, 0.8, 0.3, -0.98, 0.4, 0.3, -0.98, 0.4, -0.3]
    sd.meshes.append(scenes.MeshData("Light2", np.asarray(quad, np.float32).reshape(4, 3), np.asarray([[0, 1, 2], [0, 2, 3]], np.uint32),
                                     np.asarray([1.0, 0.0, 0.0] * 4, np.float32).reshape(4, 3), np.asarray([0, 0, 1, 0, 1, 1, 0, 1], np.float32).reshape(4, 2),
                                     scenes.matte((0.0, 0.0, 0.0)), (4.0, 6.0, 9.0)))
    return sd


def black_walls(sd):
    """Every surface black (the lights' own BSDF is black already): no light path and no camera path continues past a surface."""
    for m in sd.meshes:
        m.bsdf = scenes.matte((0.0, 0.0, 0.0))
    return sd


def two_lights(w, h):
    """The box with its medium plus the second emissive quad of add_second_light."""
    return add_second_light(scenes.cbox_medium(w, h, 1.0))


def single_bsdf(w, h, bsdf):
    sd = scenes.cbox(w, h)
    for m in sd.meshes:
        m.bsdf = bsdf
    return sd


def glass_and_mirror(w, h):
    # several BSDF types in one scene (the run-time switch); glass transmission carries eta^2 into the russian roulette
    sd = scenes.cbox(w, h)
    sd.meshes[5].bsdf = scenes.Bsdf(type=scenes.GLASS)                                                   # the short box
    sd.meshes[6].bsdf = scenes.Bsdf(type=scenes.METAL, specular=scenes.const_color((1, 1, 1)), distribution=scenes.MF_NONE)   # the tall box
    return sd
