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


def open_floor(w, h, bsdf=None, environment=None, light=True, light_in_view=False):
    """An open receiver: a camera 3 above an 8 x 8 floor looks straight down (40 degrees across), a 0.6 x 0.5 light 2 above the floor and a black occluding
    quad 1 above it both stand beside the frustum, and the occluder's shadow falls into the frame.  Nothing in view has a silhouette.
    light_in_view: the light hangs 1.5 above the floor inside the frustum instead, so that the camera sees its back (the one surface kind that is not
    turned towards the viewer), and a black canopy beside the frustum, 0.7 above the light, hides part of the sky over that back."""
    black = scenes.matte((0.0, 0.0, 0.0))
    meshes = [scenes._quad_mesh("Floor", [-4, 0, -4, -4, 0, 4, 4, 0, 4, 4, 0, -4], [0, 1, 0], bsdf or scenes.matte((0.7, 0.5, 0.3))),
              scenes._quad_mesh("Occluder", [0.9, 1, 0.0, 1.4, 1, 0.0, 1.4, 1, 0.6, 0.9, 1, 0.6], [0, 1, 0], black)]
    if light_in_view:
        meshes.append(scenes._quad_mesh("Light", [-0.1, 1.5, -0.15, 0.5, 1.5, -0.15, 0.5, 1.5, 0.35, -0.1, 1.5, 0.35], [0, -1, 0], black, emission=(9.0, 7.0, 5.0)))
        meshes.append(scenes._quad_mesh("Canopy", [0.4, 2.2, -0.4, 1.2, 2.2, -0.4, 1.2, 2.2, 0.6, 0.4, 2.2, 0.6], [0, -1, 0], black))
    elif light:
        meshes.append(scenes._quad_mesh("Light", [1.7, 2, 0.25, 2.3, 2, 0.25, 2.3, 2, 0.75, 1.7, 2, 0.75], [0, -1, 0], black, emission=(9.0, 7.0, 5.0)))
    to_world = np.asarray([1, 0, 0, 0, 0, 0, -1, 0, 0, -1, 0, 0, 0, 3, 0, 1], dtype=np.float32)
    sd = scenes.SceneData(w, h, 40.0, 0, to_world, False, meshes)
    sd.environment = environment
    return sd


def glass_and_mirror(w, h):
    # several BSDF types in one scene (the run-time switch); glass transmission carries eta^2 into the russian roulette
    sd = scenes.cbox(w, h)
    sd.meshes[5].bsdf = scenes.Bsdf(type=scenes.GLASS)                                                   # the short box
    sd.meshes[6].bsdf = scenes.Bsdf(type=scenes.METAL, specular=scenes.const_color((1, 1, 1)), distribution=scenes.MF_NONE)   # the tall box
    return sd
