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
