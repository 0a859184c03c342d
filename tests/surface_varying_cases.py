"""The cases of tests/test_surface_quadrature_varying.py (the CPU oracle) and tests/test_gpu_surface_quadrature_varying.py (the device): what varies over a
surface or over the sphere (textures, lights whose emission depends on uv, the environment map) and the light tree, each held to
tests/surface_quadrature.py (a plain module: `from tests import surface_varying_cases`).  Both files run the same list with the same seeds, counts and
check; only the renderer differs, and the oracle is bit-identical to the device.

Frame 24 x 18, K = 8 seeds, Q.check_ratios / Q.check_footprint unchanged: SE(r) <= 5 % and |mean(r) - 1| <= 4 SE + the quadrature's own error estimate.  A
channel whose reference is exactly zero (HSV's blue) has no ratio: the image's channel is asserted to be exactly zero on the kept pixels and the
others are checked.  Masks are functions of the rays alone and at most 10 % of the pixels (asserted).

Scenes.
    floor:*     tests.scene_helpers.open_floor with a texture on the floor: a checkerboard of scale (4, 3) (five edges in view), a grid whose two
                readings of scale_v differ in view, a Phong lobe over the checkerboard, and a random 4 x 3 bitmap on a floor whose uv run to 4,
                so that the frame crosses a wrap.
    box:*       the Cornell box with the triangle behind the camera, its light switched to HSV or to a 2 x 2 bitmap (scenes.override_light_emission).
    sky:*       open_floor under scenes.sky_map(8, 4) (a bright texel, a black row, a black column), with and without the rectangular light.
    tree / list scenes.many_lights(n = 3): the box under a 3 x 3 grid of tilted quads whose power varies over two decades, with and without the light tree.
                The quads hang 0.05 under a ceiling in view and NEAR takes the ceiling about them: 29 of 432 pixels, 6.7 %, within the 10 %.  Their
                normals point straight down while their planes tilt by 23 degrees, and part of the walls lies in the wedge between: `path` under "all"
                and "bsdf" lights it (surface_quadrature's path_emitting_side), asserted to miss the one-sided reference under "all" and held to the
                shading side under "bsdf" on the pixels where the two differ.
    tree-floor / list-floor  tests.scene_helpers.lights_over_floor, the same grid over open_floor: no receiver in view lies in a wedge, and `path` under
                "all" holds with and without the tree.

The counts are constants chosen on the CPU from the oracle's spread; what each case reaches is in profiles/surface_varying_note.md."""
import time

import numpy as np

from oracle import orc
from rustlight_amd import api, scenes
from tests import surface_quadrature as Q
from tests.scene_helpers import context, lights_over_floor, open_floor, with_back_triangle

W, H, K = 24, 18, 8
SEED = 4000                                          # seed k looks through the block seeds of SEED + k
FUSED, WAVEFRONT, AUTO = api.PIPELINE_FUSED, api.PIPELINE_WAVEFRONT, api.PIPELINE_AUTO
PER_SAMPLE, REFERENCE_ORDER, STRATIFIED = api.STREAM_PER_SAMPLE, api.STREAM_REFERENCE_ORDER, api.STREAM_STRATIFIED
STRATEGY = {"all": api.STRATEGY_ALL, "bsdf": api.STRATEGY_BSDF, "emitter": api.STRATEGY_EMITTER}

CHECKER = {"type": scenes.TEX_CHECKERBOARD, "color0": (0.7, 0.5, 0.3), "color1": (0.2, 0.3, 0.6), "scale": (4.0, 3.0), "offset": (0.1, 0.2)}
# in view u, v run over 0.36 .. 0.64: a line at 4 u = 2 under either reading, a line at v + 0.45 = 1 under "added" and none at 0.45 v under "multiplied"
GRID = {"type": scenes.TEX_GRID, "color0": (0.1, 0.2, 0.7), "color1": (0.7, 0.5, 0.3), "scale": (4.0, 0.45), "offset": (0.0, 0.0), "line_width": 0.1}
FLOOR_BSDFS = {
    "checker": scenes.Bsdf(type=scenes.DIFFUSE, diffuse=CHECKER),
    "grid": scenes.Bsdf(type=scenes.DIFFUSE, diffuse=GRID),
    "phong": scenes.Bsdf(type=scenes.PHONG, exponent=30.0, diffuse=CHECKER, specular=scenes.const_color((0.2, 0.3, 0.5)), weight_specular=0.5),
}
FLOOR_BITMAP = (4, 3, np.random.default_rng(7).uniform(0.05, 0.9, (3, 4, 3)).astype(np.float32))
LIGHT_BITMAP = (2, 2, np.asarray([[[9.0, 2.0, 1.0], [1.0, 8.0, 2.0]], [[2.0, 1.0, 9.0], [6.0, 6.0, 1.0]]], np.float32))
SKY_MAP = (8, 4)
FLOOR_RULE = (2, 3)                                  # the light's grid under a textured floor's Footprint


def _seeds(k):
    return orc.block_seeds(SEED + k, W, H)


def scene(name):
    """The SceneData of a case's scene; a new one at every call."""
    kind, _, what = name.partition(":")
    if kind == "floor" and what == "bitmap":
        sd = open_floor(W, H, bsdf=scenes.Bsdf(type=scenes.DIFFUSE, diffuse={"type": scenes.TEX_BITMAP, "color0": (0.0, 0.0, 0.0), "bitmap_id": 0}))
        sd.meshes[0].uv = (4.0 * sd.meshes[0].uv).astype(np.float32)
        sd.bitmaps = [FLOOR_BITMAP]
        return sd
    if kind == "floor":
        return open_floor(W, H, bsdf=FLOOR_BSDFS[what])
    if kind == "box":
        sd = with_back_triangle(scenes.cbox(W, H))
        if what == "texture":
            sd.bitmaps = [LIGHT_BITMAP]
        return scenes.override_light_emission(sd, what, 0 if what == "texture" else -1)
    if kind == "sky":
        sd = open_floor(W, H, light=what == "light")
        sd.environment_map = scenes.sky_map(*SKY_MAP)
        return sd
    if kind in ("tree-floor", "list-floor"):
        return lights_over_floor(W, H, use_ats=kind == "tree-floor")
    assert kind in ("tree", "list")
    return scenes.many_lights(W, H, n=3, use_ats=kind == "tree")


STRATEGY_VARIANTS = ("bsdf", "emitter", "all:power", "all:balance")


def _strategies(sc, sd, which, **kw):
    """fn(o, d, res) -> [4, n_rays, 3]: Q.radiance under each of STRATEGY_VARIANTS, `which` ("lights" or "sky") being the switch they turn."""
    def fn(o, d, res):
        out = []
        for variant in STRATEGY_VARIANTS:
            strategy, _, heuristic = variant.partition(":")
            out.append(Q.radiance(sc, sd, o, d, res, **{which: strategy}, heuristic=heuristic or "balance", **kw))
        return np.stack(out)
    return fn


class References:
    """The quadratures, (Footprint, variant names) per scene, each computed once and left unchanged."""

    def __init__(self):
        self._made, self.seconds = {}, {}

    def get(self, name):
        kind = name.partition(":")[0]
        key = "lights" if kind in ("tree", "list") else "lights-floor" if kind in ("tree-floor", "list-floor") else "floor" if name in ("floor:checker", "floor:grid", "floor:phong") else name
        if key not in self._made:
            start = time.time()
            sd = scene({"lights": "tree", "lights-floor": "tree-floor", "floor": "floor:checker"}.get(key, name))
            sc = orc.Scene(sd)
            if key == "floor":
                # texture edges cross pixels: 8 x 8 against 16 x 16 rays per pixel, and 6 x 6 against 12 x 12 points on the light (at 4 x 4 rays and
                # 2 x 2 points the blue channel's two differences cancelled to 0.17 % where the value was 0.41 % off the finer rule's)
                published = dict(Q.REFERENCE, grid_v_scale="multiplied")
                fn = lambda o, d, res: np.concatenate([Q.radiance(sc, sd, o, d, res, bsdfs=list(FLOOR_BSDFS.values()), rule=FLOOR_RULE),
                                                       Q.radiance(sc, sd, o, d, res, bsdfs=[FLOOR_BSDFS["grid"]], rule=FLOOR_RULE, departures=published)])
                made = Q.Footprint(sc, sd, 8, fn), list(FLOOR_BSDFS) + ["grid:published"]
            elif key == "floor:bitmap":
                made = Q.Footprint(sc, sd, 8, lambda o, d, res: Q.radiance(sc, sd, o, d, res, rule=FLOOR_RULE)[None]), ["bitmap"]
            elif kind == "box":
                # the box's rays per pixel; (2, 2) keeps the panel count on the light even, so that the 2 x 2 bitmap's texel edges under true uv are panel
                # edges at every resolution (under normalised uv they are rays through the uv origin: UvLight.sector_grid follows them)
                made = Q.Footprint(sc, sd, 8, _strategies(sc, sd, "lights", rule=(2, 2))), list(STRATEGY_VARIANTS)
            elif kind == "sky":
                made = Q.Footprint(sc, sd, 4, _strategies(sc, sd, "sky", rule=Q.FOOTPRINT_RULE)), list(STRATEGY_VARIANTS)
            elif key == "lights":
                fn = lambda o, d, res: np.stack([Q.radiance(sc, sd, o, d, res, rule=Q.FOOTPRINT_RULE, hit_side=side) for side in ("geometric", "shading")])
                made = Q.Footprint(sc, sd, 8, fn), ["lights", "lights:path-bsdf"]
            else:
                made = Q.Footprint(sc, sd, 4, lambda o, d, res: Q.radiance(sc, sd, o, d, res, rule=Q.FOOTPRINT_RULE)[None]), ["lights"]
            assert made[0].keep.mean() >= 0.9, "more than 10 % of the pixels masked"
            self.seconds[key] = time.time() - start
            print(f"reference {key}: {int((~made[0].keep).sum())} of {W * H} pixels masked, {self.seconds[key]:.1f} s")
            self._made[key] = made
        return self._made[key]


class _Channels:
    """A Footprint seen through some of its colour channels."""

    def __init__(self, fp, channels):
        self.fp, self.channels, self.keep = fp, channels, fp.keep

    def mean(self, also=None):
        return tuple(v[:, self.channels] for v in self.fp.mean(also))


def check(label, images, reference, name, also=None, expect_miss=False):
    """Q.check_footprint over the channels in which the reference is not exactly zero; in the others every image is asserted to be exactly zero on the
    kept pixels."""
    fp, names = reference
    value = fp.mean(also)[0][names.index(name)]
    keep = fp.keep if also is None else fp.keep & also
    lit = np.nonzero(value != 0.0)[0]
    for c in np.nonzero(value == 0.0)[0]:
        assert not any(img[keep][:, c].any() for img in images), (label, "channel", int(c), "is black in the reference and not in the image")
    return Q.check_footprint(label, [img[..., lit] for img in images], (_Channels(fp, lit), names), name, also=also, expect_miss=expect_miss)


def lit_columns():
    lit = np.zeros((H, W), bool)
    lit[:, :W - (W - H) // 2] = True                                  # Camera::importance's `p.x > image_rect_max.y`: columns 21 .. 23 get none
    return lit


# ---- the renderers
class Oracle:
    """The CPU oracle.  It has one pipeline and one way to hold a scene: cases that differ in those alone share their images."""
    name = "oracle"

    def __init__(self):
        self._scenes, self._images = {}, {}

    def _scene(self, name):
        if name not in self._scenes:
            self._scenes[name] = orc.Scene(scene(name))
        return self._scenes[name]

    def _once(self, key, render):
        if key not in self._images:
            self._images[key] = [render(k) for k in range(K)]
        return self._images[key]

    def direct(self, name, nb, spp, stream_mode=PER_SAMPLE):
        sc = self._scene(name)
        return self._once((name, "direct", nb, spp, stream_mode), lambda k: sc.render_direct(seeds=_seeds(k), spp=spp, nb_bsdf_samples=nb[0], nb_light_samples=nb[1],
                                                                                             stream_mode=stream_mode)[0])

    def path(self, name, strategy, spp, max_depth=3, pipeline=AUTO, stream_mode=PER_SAMPLE, streaming=False):
        sc = self._scene(name)
        return self._once((name, "path", strategy, spp, max_depth, stream_mode),
                          lambda k: sc.render(seeds=_seeds(k), spp=spp, max_depth=max_depth, strategy=STRATEGY[strategy], stream_mode=stream_mode)[0])

    def light(self, name, spp, max_depth=2):
        def render(k):
            img, st = self._scene(name).render_light(seeds=_seeds(k), spp=spp, max_depth=max_depth)
            assert st["splats_invalid"] == 0 and st["splats_saturated"] == 0
            return img
        return self._once((name, "light", spp, max_depth), render)


class Device:
    """The device through rustlight_amd.api."""
    name = "device"

    def __init__(self):
        self._contexts = {}

    def _context(self, name, streaming=False):
        if (name, streaming) not in self._contexts:
            self._contexts[name, streaming] = context(scene(name), streaming=streaming)
        return self._contexts[name, streaming]

    def direct(self, name, nb, spp, stream_mode=PER_SAMPLE):
        ctx = self._context(name)
        return [ctx.render_direct(_seeds(k), spp=spp, nb_bsdf_samples=nb[0], nb_light_samples=nb[1], stream_mode=stream_mode)[0] for k in range(K)]

    def path(self, name, strategy, spp, max_depth=3, pipeline=AUTO, stream_mode=PER_SAMPLE, streaming=False):
        ctx = self._context(name, streaming)
        params = dict(max_depth=max_depth, strategy=STRATEGY[strategy], pipeline=pipeline, stream_mode=stream_mode)
        return [ctx.render(_seeds(k), api.path_params(spp, **params))[0] for k in range(K)]

    def light(self, name, spp, max_depth=2):
        images = []
        for k in range(K):
            img, st = self._context(name).render_light(_seeds(k), spp=spp, max_depth=max_depth)
            assert st["splats_invalid"] == 0 and st["splats_saturated"] == 0
            images.append(img)
        return images


# ---- the cases: (id, scene, what renders it (method, arguments), reference variant, keywords of check)
SPP_DIRECT = {(0, 1): 64, (1, 0): 256, (1, 1): 64}
SPP_PATH = 256
SPP_LIGHT = 256
SPP_WEDGE = 8192                                     # path under "bsdf" on the pixels of the wedge: sampled directions find lights of 0.12 x 0.12 (against the
                                                     # one-sided reference, which is the smaller, SE 7 % at 1024 and 5.2 % at 4096)
NB = [(0, 1), (1, 0), (1, 1)]
PIPELINES = {"wavefront": dict(pipeline=WAVEFRONT), "fused": dict(pipeline=FUSED)}
PURE = {(0, 1): "emitter", (1, 0): "bsdf"}


def _nb(nb):
    return f"{nb[0]}{nb[1]}"


def _cases():
    out = []

    def add(name, scene_name, how, variant, **kw):
        out.append((name, scene_name, how, variant, kw))

    # textured albedo
    for tex in ("checker", "bitmap", "grid", "phong"):
        for nb in NB:
            add(f"direct-{tex}-{_nb(nb)}", f"floor:{tex}", ("direct", dict(nb=nb, spp=SPP_DIRECT[nb])), tex)
    add("direct-grid-11-published-misses", "floor:grid", ("direct", dict(nb=(1, 1), spp=SPP_DIRECT[1, 1])), "grid:published", expect_miss=True)
    for pipe, kw in PIPELINES.items():
        add(f"path-checker-{pipe}", "floor:checker", ("path", dict(strategy="all", spp=SPP_PATH, **kw)), "checker")
    # lights whose emission depends on uv
    for light in ("hsv", "texture"):
        box = f"box:{light}"
        add(f"direct-{light}-01", box, ("direct", dict(nb=(0, 1), spp=SPP_DIRECT[0, 1])), "emitter")
        add(f"direct-{light}-10", box, ("direct", dict(nb=(1, 0), spp=SPP_DIRECT[1, 0])), "bsdf")
        add(f"direct-{light}-11", box, ("direct", dict(nb=(1, 1), spp=SPP_DIRECT[1, 1])), "all:power")
        add(f"direct-{light}-01-told-apart", box, ("direct", dict(nb=(0, 1), spp=SPP_DIRECT[0, 1])), "bsdf", expect_miss=True)
        for strategy in ("all", "bsdf", "emitter"):
            variant = "all:balance" if strategy == "all" else strategy
            add(f"path-{light}-{strategy}-reference-order", box, ("path", dict(strategy=strategy, spp=SPP_PATH, stream_mode=REFERENCE_ORDER)), variant)
            add(f"path-{light}-{strategy}-streamed", box, ("path", dict(strategy=strategy, spp=SPP_PATH, streaming=True)), variant)
        # the light tracer leaves from sampled points (src/integrators/explicit/light.rs with Mesh::sample_tri, geometry.rs:317-326): Le(uv / |uv|)
        add(f"light-tracing-{light}", box, ("light", dict(spp=SPP_LIGHT)), "emitter", also="lit_columns")
        add(f"light-tracing-{light}-told-apart", box, ("light", dict(spp=SPP_LIGHT)), "bsdf", also="lit_columns", expect_miss=True)
    # the environment map
    for sky in ("sky:alone", "sky:light"):
        tag = sky.replace(":", "-")
        for nb in NB:
            add(f"direct-{tag}-{_nb(nb)}", sky, ("direct", dict(nb=nb, spp=SPP_DIRECT[nb])), PURE.get(nb, "all:power"))
    add("direct-sky-alone-01-told-apart", "sky:alone", ("direct", dict(nb=(0, 1), spp=SPP_DIRECT[0, 1])), "bsdf", expect_miss=True)
    for strategy in ("all", "bsdf", "emitter"):
        for pipe, kw in PIPELINES.items():
            add(f"path-sky-light-{strategy}-{pipe}", "sky:light", ("path", dict(strategy=strategy, spp=SPP_PATH, **kw)), "all:balance" if strategy == "all" else strategy)
    # the light tree, and beside it the same cases without it
    for scene_name in ("tree", "list"):
        add(f"direct-{scene_name}-01", scene_name, ("direct", dict(nb=(0, 1), spp=SPP_DIRECT[0, 1])), "lights")
        add(f"direct-{scene_name}-11", scene_name, ("direct", dict(nb=(1, 1), spp=SPP_DIRECT[1, 1])), "lights")
        add(f"direct-{scene_name}-01-stratified", scene_name, ("direct", dict(nb=(0, 1), spp=SPP_DIRECT[0, 1], stream_mode=STRATIFIED)), "lights")
        for pipe, kw in PIPELINES.items():
            add(f"path-{scene_name}-emitter-{pipe}", scene_name, ("path", dict(strategy="emitter", spp=SPP_PATH, **kw)), "lights")
            # path_emitting_side: under "all" the wedge between a tilted quad's plane and the plane of its normals is lit, against the one-sided reference
            add(f"path-{scene_name}-all-{pipe}-misses-one-side", scene_name, ("path", dict(strategy="all", spp=SPP_PATH, **kw)), "lights", expect_miss=True)
            add(f"path-{scene_name}-floor-all-{pipe}", f"{scene_name}-floor", ("path", dict(strategy="all", spp=SPP_PATH, **kw)), "lights")
    # sampled directions make no use of the tree: once
    add("path-list-bsdf-shading-side", "list", ("path", dict(strategy="bsdf", spp=SPP_WEDGE)), "lights:path-bsdf", also="wedge")
    add("path-list-bsdf-one-side-misses", "list", ("path", dict(strategy="bsdf", spp=SPP_WEDGE)), "lights", also="wedge", expect_miss=True)
    return out


CASES = _cases()
CASE_IDS = [c[0] for c in CASES]


def run(case, renderer, references):
    """Render the case's K images with `renderer` and check them; `path` is first held to its gate: at max_depth = 2 the kept pixels are black."""
    name, scene_name, (how, args), variant, kw = case
    reference = references.get(scene_name)
    kw = dict(kw)
    if kw.get("also") == "lit_columns":
        kw["also"] = lit_columns()
    elif kw.get("also") == "wedge":                                      # the pixels whose two references differ by more than a fifth: a function of the rays
        one, shading = (reference[0].image(reference[1].index(v)) @ Q.LUMINANCE for v in ("lights", "lights:path-bsdf"))
        kw["also"] = shading > 1.2 * one
        assert (kw["also"] & reference[0].keep).sum() >= 12, "the wedge fills too few pixels"
    if how == "path":
        below = getattr(renderer, how)(scene_name, **dict(args, spp=4, max_depth=2))
        assert not any(img[reference[0].keep].any() for img in below), (name, "max_depth = 2 is not emission alone")
    start = time.time()
    images = getattr(renderer, how)(scene_name, **args)
    seconds = time.time() - start
    if how == "light":
        assert not any(img[~lit_columns()].any() for img in images)
    mean, se, margin = check(f"{renderer.name} {name}", images, reference, variant, **kw)
    print(f"{renderer.name} {name}: {seconds:.2f} s to render")
    return mean, se, margin
