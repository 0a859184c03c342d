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


def lights_over_floor(w, h, n=3, use_ats=True):
    """open_floor without its light under scenes.many_lights' n x n grid of small tilted quads whose emission varies over two decades, 2 above the floor and
    beside the frustum (x 0.6 .. 2.4, z -0.9 .. 0.9): the many-light case with no ceiling and no silhouette in view; the occluder shadows some of them."""
    sd = open_floor(w, h, light=False)
    for i in range(n):
        for j in range(n):
            cx, cz, half = 0.6 + 1.8 * (i + 0.5) / n, -0.9 + 1.8 * (j + 0.5) / n, 0.06
            tilt = 0.05 * ((i + 2 * j) % 3 - 1)
            e = 0.5 * (1.0 + ((7 * i + 3 * j) % 11)) ** 2 / 4.0
            corners = [cx - half, 2.0 + tilt, cz - half, cx + half, 2.0 - tilt, cz - half, cx + half, 2.0 - tilt, cz + half, cx - half, 2.0 + tilt, cz + half]
            sd.meshes.append(scenes._quad_mesh(f"L{i * n + j}", corners, [0, -1, 0], scenes.matte((0.0, 0.0, 0.0)), emission=(e, 0.8 * e, 0.5 * e)))
    sd.use_ats = use_ats
    return sd


RECEIVER_ALBEDO = (0.7, 0.5, 0.3)
RECEIVERS = [  # (point, normal): below and beside the light at different distances and tilts, every one with the whole light above its horizon
    ((0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), ((0.9, 0.3, -0.4), (-0.3, 1.0, 0.2)), ((-1.2, 1.0, 0.6), (1.0, 0.4, -0.2)), ((0.2, 1.5, 0.1), (0.1, 1.0, -0.1)),
    ((1.5, -0.5, 1.0), (-0.5, 1.0, -0.5)), ((-0.3, 1.75, -0.2), (0.0, 1.0, 0.0))]


def receiver_scene(which, light_quad, emission=(3.0, 2.0, 1.0), lights=(), normals_on_receivers=False):
    """A quad light facing down and receiver `which` of RECEIVERS, a small triangle with or without shading normals, alone: no receiver shadows another."""
    meshes = [scenes._quad_mesh("light", light_quad, [0, -1, 0], scenes.matte((0, 0, 0)), emission=emission)]
    for p, n in RECEIVERS[which:which + 1]:
        p, n = np.asarray(p, np.float64), np.asarray(n, np.float64) / np.linalg.norm(n)
        s = np.cross(n, [0.0, 0.0, 1.0] if abs(n[2]) < 0.9 else [1.0, 0.0, 0.0])
        s /= np.linalg.norm(s)
        t = np.cross(n, s)
        tri = np.asarray([p + 0.01 * s, p - 0.005 * s + 0.009 * t, p - 0.005 * s - 0.009 * t], np.float32)
        meshes.append(scenes.MeshData("receiver", tri, np.asarray([[0, 1, 2]], np.uint32), np.tile(-n, (3, 1)).astype(np.float32) if normals_on_receivers else None,
                                      None, scenes.matte(RECEIVER_ALBEDO)))
    to_world = np.asarray([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, -5, 1], dtype=np.float32)
    sd = scenes.SceneData(8, 8, 40.0, 0, to_world, False, meshes)
    sd.lights = list(lights)
    return sd


def ray_at_receiver(which):
    """A ray at the receiver's centre, from its normal's side at a slant."""
    p, n = (np.asarray(a, np.float64) for a in RECEIVERS[which])
    start = p + 0.2 * n / np.linalg.norm(n) + 0.1 * np.cross(n / np.linalg.norm(n), [0.3, 0.5, 0.8])
    return start[None, :], ((p - start) / np.linalg.norm(p - start))[None, :]


DELTA_SKY = (0.3, 0.4, 0.6)
MIRROR_TILT = 55.0
PANE_HALF = 4.0
MIRROR_CENTRE, MIRROR_HALF = (0.3, 1.3, 0.4), 0.5


def flat_quad(name, x0, x1, y, z0, z1, up, bsdf):
    """A quad in the plane of height y whose mesh normal, in the normals array and by its winding alike, points up or down."""
    corners = [x0, y, z0, x0, y, z1, x1, y, z1, x1, y, z0]
    if not up:
        corners = [x0, y, z0, x1, y, z0, x1, y, z1, x0, y, z1]
    return scenes._quad_mesh(name, corners, [0, 1 if up else -1, 0], bsdf)


def pane(w, h, camera_inside=False, tilt=0.0):
    """open_floor under a sky with an 8 x 8 pane of glass 2.5 above the floor, between the camera (3 above) and everything else: a single crossing, the one
    place where the eta^2 of radiance does not cancel.  camera_inside: the pane's normal points down, so that the camera looks out of the denser side.
    tilt: the camera turned by that many degrees towards +x about its own vertical axis; with camera_inside and 41.6 degrees the frame's 40 degrees
    straddle the critical angle asin(1 / eta)."""
    sd = open_floor(w, h, environment=DELTA_SKY)
    sd.meshes.append(flat_quad("Pane", -PANE_HALF, PANE_HALF, 2.5, -PANE_HALF, PANE_HALF, not camera_inside, scenes.Bsdf(type=scenes.GLASS)))
    c, s = np.cos(np.radians(tilt)), np.sin(np.radians(tilt))
    sd.to_world = np.asarray([c, s, 0, 0, 0, 0, -1, 0, s, -c, 0, 0, 0, 3, 0, 1], dtype=np.float32)
    if tilt:
        # what the pane reflects past the critical angle ends on a black canopy 0.9 above it, what it reflects short of that angle passes the canopy's edge
        # into the sky: under a sky alone a ray sent on along the pane instead of back up would find the same radiance
        sd.meshes.append(flat_quad("Canopy", 1.3, 4, 3.4, -2, 2, False, scenes.matte((0.0, 0.0, 0.0))))
    return sd


def slab(w, h):
    """open_floor under a sky with a slab of glass between the camera and everything else: two 8 x 8 quads 2.5 and 2.2 above the floor, normals outward."""
    sd = open_floor(w, h, environment=DELTA_SKY)
    sd.meshes.append(flat_quad("SlabTop", -PANE_HALF, PANE_HALF, 2.5, -PANE_HALF, PANE_HALF, True, scenes.Bsdf(type=scenes.GLASS)))
    sd.meshes.append(flat_quad("SlabBottom", -PANE_HALF, PANE_HALF, 2.2, -PANE_HALF, PANE_HALF, False, scenes.Bsdf(type=scenes.GLASS)))
    return sd


def mirror(w, h, shows_light=False):
    """open_floor (no sky: by way of a mirror a sky lights the floor from a whole hemisphere of images, which no image source sums up) with a smooth-metal
    quad (the default eta and k: three different Fresnel curves) 1.6 x 1.2, tilted in view about the z axis: it covers the left of the frame and reflects
    the lit floor.  shows_light: a quad of side 2 MIRROR_HALF about MIRROR_CENTRE instead, turned so that the camera sees the light's centre in its own."""
    sd = open_floor(w, h)
    metal = scenes.Bsdf(type=scenes.METAL, distribution=scenes.MF_NONE)
    if shows_light:
        # the mirror's plane passes through MIRROR_CENTRE with normal n = unit(d_light - d_camera) for the light's centre (2, 2, 0.5): the camera sees it there
        centre, to_camera, to_light = np.asarray(MIRROR_CENTRE), np.asarray([0.0, 3.0, 0.0]), np.asarray([2.0, 2.0, 0.5])
        a, b = to_camera - centre, to_light - centre
        n = a / np.linalg.norm(a) + b / np.linalg.norm(b)
        n /= np.linalg.norm(n)
        s = np.cross([0.0, 0.0, 1.0], n)
        s /= np.linalg.norm(s)
        t = np.cross(n, s)
        corners = [centre + MIRROR_HALF * (i * s + j * t) for i, j in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
    else:
        c, s = np.cos(np.radians(MIRROR_TILT)), np.sin(np.radians(MIRROR_TILT))
        n = np.asarray([s, c, 0.0])
        corners = [np.asarray([-0.5 + i * 0.8 * c, 0.8 - i * 0.8 * s, 0.6 * j]) for i, j in ((-1, -1), (-1, 1), (1, 1), (1, -1))]
    sd.meshes.append(scenes._quad_mesh("Mirror", np.concatenate(corners).tolist(), [float(x) for x in n], metal))
    return sd


def coat(w, h):
    """open_floor under a sky, its floor a smooth substrate: a diffuse term under a mirror coat of Schlick's F."""
    return open_floor(w, h, environment=DELTA_SKY,
                      bsdf=scenes.Bsdf(type=scenes.SUBSTRATE, diffuse=scenes.const_color((0.5, 0.3, 0.2)), specular=scenes.const_color((0.05, 0.05, 0.05)),
                                       distribution=scenes.MF_NONE))


def caustic(w, h):
    """open_floor with an upright smooth-metal quad in the plane x = -1.3, beside the frustum and facing the light: it throws the light's image onto the
    floor in view, the occluder's shadow included, where nothing else lights the floor."""
    sd = open_floor(w, h)
    sd.meshes.append(scenes._quad_mesh("Mirror", [-1.3, 0.02, -1.5, -1.3, 2.5, -1.5, -1.3, 2.5, 2.5, -1.3, 0.02, 2.5], [1, 0, 0],
                                       scenes.Bsdf(type=scenes.METAL, distribution=scenes.MF_NONE)))
    return sd


def lit_through_a_pane(w, h):
    """open_floor with a pane of glass 1.5 above the floor under the light, x 0.7 .. 3.3, z -0.8 .. 1.8, normal up, beside the frustum: every segment from the
    floor in view to the light crosses it, so a light sample finds nothing and the floor is lit through one crossing alone, which `path` and the light
    tracer can both render."""
    sd = open_floor(w, h)
    sd.meshes.append(flat_quad("Pane", 0.7, 3.3, 1.5, -0.8, 1.8, True, scenes.Bsdf(type=scenes.GLASS)))
    return sd


# name: (builder(w, h), the delta tree's max_edges, rays per pixel n of the reference: n x n against 2n x 2n; a mirror's outline in view needs more).  `path` renders exactly the tree's paths at max_depth = max_edges + 1: one more and the first path with
# two vertices that are no delta vertices comes in (floor -> pane -> sky, floor -> mirror -> floor, a coat's second bounce).
DELTA_SCENES = {
    "pane": (lambda w, h: pane(w, h), 3, 2),                                                  # camera -> pane -> floor -> light
    "pane_inside": (lambda w, h: pane(w, h, camera_inside=True), 3, 2),
    "pane_critical": (lambda w, h: pane(w, h, camera_inside=True, tilt=41.6), 3, 4),
    "slab": (lambda w, h: slab(w, h), 4, 2),                                                  # camera -> top -> bottom -> floor -> light
    "mirror": (lambda w, h: mirror(w, h), 3, 4),                                              # camera -> mirror -> floor -> light
    "mirror_light": (lambda w, h: mirror(w, h, shows_light=True), 3, 4),
    "caustic": (lambda w, h: caustic(w, h), 3, 2),                                         # camera -> floor -> mirror -> light: the image source
    "coat": (lambda w, h: coat(w, h), 2, 2),                                                  # camera -> coat -> light or sky
}


def glass_and_mirror(w, h):
    # several BSDF types in one scene (the run-time switch); glass transmission carries eta^2 into the russian roulette
    sd = scenes.cbox(w, h)
    sd.meshes[5].bsdf = scenes.Bsdf(type=scenes.GLASS)                                                   # the short box
    sd.meshes[6].bsdf = scenes.Bsdf(type=scenes.METAL, specular=scenes.const_color((1, 1, 1)), distribution=scenes.MF_NONE)   # the tall box
    return sd
