"""The surface integrators on the device (direct, path, light-tracing, ao) held to tests/surface_quadrature.py, the float64 direct-lighting quadrature that
shares no shading code with the kernels or the oracle (tests/test_surface_quadrature.py holds the quadrature itself to closed forms).  A term that kernel and
oracle both read wrongly from the reference's text (a BSDF's normalisation, a cosine, the Fresnel term, the microfacet Jacobian, the area -> solid-angle
conversion, a point light's 1 / r^2, direct's 1 / nb, the light tracer's importance) passes every bit-exact test and fails here.

Frame 24 x 18 (2 x 2 blocks, both edges ragged).  The statistic is volume_quadrature.check_ratios over K = 8 seeds: r_k = mean(image_k) / mean(quadrature), one
ratio per seed and channel over the kept pixels; asserted SE(r) <= 5 % and |mean(r) - 1| <= 4 SE(r) + the quadrature's error (resolution 2 against 1, plus
16 x 16 against 8 x 8 rays per pixel).  Masks are functions of the rays alone: a pixel is left out if one of its rays sees a light or ends within NEAR of one;
at most 10 % may be masked (asserted; the box loses 6 pixels of 432).  Pixels that look past the scene stay in, zero on both sides.

Scenes: the Cornell box with the triangle behind the camera (with_back_triangle: the light tracer's connections need the root box to reach the camera), its
own three Lambert albedos or one of surface_quadrature.TEST_BSDFS on every mesh; and tests.scene_helpers.open_floor, a floor that fills the frame under a
rectangular light and an occluding quad, with no silhouette in view.

Depth gates (each confirmed on the CPU oracle, tests/test_surface_quadrature.py): path max_depth = 3 is emission plus direct lighting (2 is emission alone,
asserted); light-tracing max_depth = 2 is light -> surface -> camera, on the W - (W - H) / 2 = 21 columns Camera::importance gives any importance
(camera.rs:130, kept; the others are black, asserted).  vpl is left out: with option_vpl = SURFACE, max_depth = 2 stores a first-bounce surface VPL beside
nearly every emitter record (direct plus one bounce, 1.43), and at max_depth = 1 the CPU oracle aborts, so no gate that was found leaves the emitter records
alone at a surface.

The quadrature computes what the reference renderer computes where that departs from the published models (surface_quadrature.REFERENCE: the Phong lobe
without its cosine, Beckmann's rational G1, the conductor Fresnel term with 2 a cos^2, and on the light tracer the Phong lobe times cos_l / cos_v).  On a rough
metal the MIS weights of direct do not sum to one (BSDFMetal::sample reports the microfacet normal's density, pdf the outgoing direction's): the pure
strategies are asserted to hold and the combinations to miss, as the CPU run shows.

Delta BSDFs (glass, the smooth metal, the smooth substrate) are held through surface_quadrature.delta_radiance, the deterministic tree a camera ray becomes
at delta vertices, on tests.scene_helpers.DELTA_SCENES (a pane of glass from either side and across the critical angle, a slab, two mirrors, the caustic of a third, a coated floor;
all on open_floor's layout).  Gates: path max_depth = max_edges + 1 renders exactly the tree's paths (one below is darker or black, asserted; one more and
the first path with two vertices that are no delta vertices comes in).  What the reference does there and the published models do not is again a switch of
the quadrature: no eta^2 on what crosses glass, the `emitter` strategy dropping whatever a delta edge finds, no light sample at a smooth substrate, and the
shadow ray of a sky sample ending short of the scene's sphere.  The light tracer is held on the caustic and, beside `path`, on a floor lit through one pane, where
the two compute different radiance scalings; vpl is not held (profiles/delta_quadrature_note.md says why).

The counts are constants chosen on the CPU from the oracle's spread (bit-identical to the device's); what each case reaches is in
profiles/surface_quadrature_note.md and profiles/delta_quadrature_note.md."""
import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import surface_quadrature as Q
from tests.scene_helpers import DELTA_SCENES, add_second_light, context as _context, lit_through_a_pane, open_floor, single_bsdf, with_back_triangle

pytestmark = pytest.mark.gpu

W, H, K = 24, 18, 8
SEED = 3000                                          # seed k looks through the block seeds of SEED + k
SKY = (0.3, 0.4, 0.6)
SPP_MIS_METAL = 512                                  # the metal's MIS excess is 0.5 .. 2 %: SE 0.03 % tells it from the margin
SPP_PATH = SPP_LIGHT = SPP_AO = 256
AO_BACK_CASES = [(None, False), (None, True), (2.0, True)]   # (max_distance, normal_correction) on the frame that shows a light's back


def _seeds(k):
    return orc.block_seeds(SEED + k, W, H)


def _box(name="lambert", second_light=False):
    sd = scenes.cbox(W, H) if name == "lambert" else single_bsdf(W, H, Q.TEST_BSDFS[name])
    if second_light:
        add_second_light(sd)
    return with_back_triangle(sd)


def _other_light(which):
    return with_back_triangle(scenes.cbox_other_lights(W, H, point=which == "point", directional=which == "directional", environment=False,
                                                       keep_area_light=False))


class _Reference:
    """The quadratures, each computed once and left unchanged."""

    def __init__(self):
        self._made = {}

    def get(self, which):
        """(Footprint, variant names)."""
        if which not in self._made:
            if which == "box":
                sd = _box()
                made = Q.box_reference(orc.Scene(sd), sd)
            elif which == "ao":
                sd = scenes.cbox(W, H)
                sc = orc.Scene(sd)
                fn = lambda o, d, res: np.repeat(Q.ambient_occlusion(sc, sd, o, d, res, max_distance=(1.0, None))[:, :, None], 3, axis=2)
                made = Q.Footprint(sc, sd, 8, fn, mask_lights=False), ["1.0", "None"]
            elif which == "ao_floor":
                sd = open_floor(W, H)
                sc = orc.Scene(sd)
                fn = lambda o, d, res: np.repeat(Q.ambient_occlusion(sc, sd, o, d, 2 * res, max_distance=(1.5, None))[:, :, None], 3, axis=2)
                made = Q.Footprint(sc, sd, 2, fn, mask_lights=False), ["1.5", "None"]
            elif which == "ao_back":
                sd = open_floor(W, H, light_in_view=True)
                made = Q.ao_reference(orc.Scene(sd), sd, 8, AO_BACK_CASES)
            else:
                sd = {"two_lights": lambda: _box(second_light=True), "point": lambda: _other_light("point"), "directional": lambda: _other_light("directional"),
                      "floor": lambda: open_floor(W, H), "floor_sky": lambda: open_floor(W, H, environment=SKY)}[which]()
                sc = orc.Scene(sd)
                # rays per pixel (n x n against 2n x 2n) and the light's grid: the floor has no silhouette in view, a shadow's edge only; the directional
                # light's hard shadow edges settle at 16 x 16 against 32 x 32 rays alone (8 x 8 against 16 x 16 left 2.2 %, now 0.04 %); the second light
                # 0.02 off its wall needs 4 x 4 against 16 x 16 points (2 x 2 against 8 x 8 left 0.65 % in blue)
                n = {"floor": 4, "floor_sky": 4, "directional": 16}.get(which, 8)
                rule = (2, 2) if which == "two_lights" else Q.FOOTPRINT_RULE
                made = Q.Footprint(sc, sd, n, lambda o, d, res: Q.radiance(sc, sd, o, d, res, rule=rule)[None]), [which]
            assert made[0].keep.mean() >= 0.9, "more than 10 % of the pixels masked"
            print(f"reference {which}: {int((~made[0].keep).sum())} of {W * H} pixels masked")
            self._made[which] = made
        return self._made[which]


@pytest.fixture(scope="module")
def reference(built):
    return _Reference()


def _check(label, images, reference, which, name, **kw):
    return Q.check_footprint(label, images, reference.get(which), name, **kw)


def _direct(ctx, nb, spp, **kw):
    return [ctx.render_direct(_seeds(k), spp=spp, nb_bsdf_samples=nb[0], nb_light_samples=nb[1], **kw)[0] for k in range(K)]


# ---- direct
@pytest.mark.parametrize("nb", [(0, 1), (1, 0), (1, 1), (2, 3)])
@pytest.mark.parametrize("name", ["lambert", "phong30", "phong5", "substrate"])
def test_direct(reference, name, nb):
    """Light sampling, BSDF sampling and their MIS where sample and pdf agree: a BSDF's normalisation and cosine, the area -> solid-angle conversion,
    1 / nb_bsdf and 1 / nb_light."""
    _check(f"direct {name} {nb}", _direct(_context(_box(name)), nb, Q.DIRECT_SPP[nb]), reference, "box", name)


@pytest.mark.parametrize("nb", [(0, 1), (1, 0)])
@pytest.mark.parametrize("name", ["beckmann", "ggx"])
def test_direct_on_a_rough_metal(reference, name, nb):
    """Either pure strategy holds: D, G, the Fresnel term (the renderer's, surface_quadrature's conductor_fresnel = "cos2") and the weight of a sampled
    microfacet normal."""
    _check(f"direct {name} {nb}", _direct(_context(_box(name)), nb, 256), reference, "box", name)


@pytest.mark.parametrize("nb", [(1, 1), (2, 3)])
@pytest.mark.parametrize("name", ["beckmann", "ggx"])
def test_direct_mis_on_a_rough_metal_misses(reference, name, nb):
    """The reference's own bias, kept and pinned: BSDFMetal::sample returns the density of the microfacet normal (metal.rs:66) where BSDFMetal::pdf returns
    that of the outgoing direction (metal.rs:107, D cos / (4 |wo . h|)), so the power heuristic's two weights do not sum to one.  On the CPU at these counts
    (1, 1) reads 1.010 (Beckmann) and 1.0056 (GGX), (2, 3) 1.021 and 1.011, each +- 0.0003: asserted to miss by more than the margin."""
    _check(f"direct {name} {nb} MIS", _direct(_context(_box(name)), nb, SPP_MIS_METAL), reference, "box", name, expect_miss=True)


def test_direct_with_two_area_lights(reference):
    """The flux cdf and n_lights: the second light emits (4, 6, 9) where the first emits (17, 12, 4), so a wrong share shows per channel."""
    sd = _box(second_light=True)
    assert len(Q.lights_of(sd)) == 2
    _check("direct two lights (1, 1)", _direct(_context(sd), (1, 1), 512), reference, "two_lights", "two_lights")


@pytest.mark.parametrize("which", ["point", "directional"])
def test_direct_with_a_point_or_a_directional_light(reference, which):
    """Each alone in the box (the quad under the ceiling emits nothing): I / r^2 and the plain cosine, with hard shadows."""
    _check(f"direct {which} light (1, 1)", _direct(_context(_other_light(which)), (1, 1), 64), reference, which, which)


@pytest.mark.parametrize("nb", [(0, 1), (1, 1)])
def test_direct_under_a_constant_sky(reference, nb):
    """The open floor under its rectangular light and a sky of (0.3, 0.4, 0.6), the occluder and the light's quad hiding part of it."""
    _check(f"direct floor + sky {nb}", _direct(_context(open_floor(W, H, environment=SKY)), nb, 128), reference, "floor_sky", "floor_sky")


def test_direct_on_the_open_floor(reference):
    _check("direct floor (1, 1)", _direct(_context(open_floor(W, H)), (1, 1), 64), reference, "floor", "floor")


@pytest.mark.parametrize("how", ["stratified", "reference_order", "streaming"])
def test_direct_through_the_other_samplers_and_the_streamed_scene(reference, how):
    """`-r stratified`, the reference-order streams (the two-pass chain form) and the scene streamed instead of staged in LDS; Phong of exponent 30, (1, 1)."""
    ctx = _context(_box("phong30"), streaming=how == "streaming")
    kw = {"stratified": dict(stream_mode=api.STREAM_STRATIFIED), "reference_order": dict(stream_mode=api.STREAM_REFERENCE_ORDER), "streaming": {}}[how]
    _check(f"direct phong30 (1, 1) {how}", _direct(ctx, (1, 1), 64, **kw), reference, "box", "phong30")


# ---- path
@pytest.mark.parametrize("pipeline,stream_mode", [(api.PIPELINE_WAVEFRONT, api.STREAM_PER_SAMPLE), (api.PIPELINE_FUSED, api.STREAM_PER_SAMPLE),
                                                  (api.PIPELINE_AUTO, api.STREAM_REFERENCE_ORDER)])
@pytest.mark.parametrize("strategy", [api.STRATEGY_ALL, api.STRATEGY_BSDF, api.STRATEGY_EMITTER])
@pytest.mark.parametrize("name", ["lambert", "phong30"])
def test_path_at_depth_three(reference, name, strategy, pipeline, stream_mode):
    fp, _ = reference.get("box")
    ctx = _context(_box(name))
    gate = dict(strategy=strategy, pipeline=pipeline, stream_mode=stream_mode)
    assert not ctx.render(_seeds(0), api.path_params(4, max_depth=2, **gate))[0][fp.keep].any()
    images = [ctx.render(_seeds(k), api.path_params(SPP_PATH, max_depth=3, **gate))[0] for k in range(K)]
    _check(f"path {name} strategy {strategy} pipeline {pipeline} streams {stream_mode}", images, reference, "box", name)


# ---- light-tracing
@pytest.mark.parametrize("name", ["lambert", "phong5"])
def test_light_tracing_at_depth_two(reference, name):
    """The camera's importance (1 / (A cos^3) / r^2) and the BSDF as the light tracer evaluates it, wo towards the camera (light.rs:100-106).  It needs
    f cos_v; phong.rs:116 puts d_out.z, there cos_v, on the diffuse part alone, so the Phong lobe lacks cos_v where under the camera-side integrators it lacks
    cos_l, and reads as the lobe times cos_l / cos_v: surface_quadrature's phong_lobe_cosine = "adjoint" (against the camera-side lobe exponent 5 reads
    1.025, 1.038, 1.057).  light.rs:107-108, the shading-normal correction, is 1 on every mesh here."""
    ctx = _context(_box(name))
    lit = np.zeros((H, W), bool)
    lit[:, :W - (W - H) // 2] = True                                  # Camera::importance's `p.x > image_rect_max.y`: columns 21 .. 23 get none
    images = []
    for k in range(K):
        img, st = ctx.render_light(_seeds(k), spp=SPP_LIGHT, max_depth=2)
        assert st["splats_invalid"] == 0 and st["splats_saturated"] == 0 and not img[~lit].any()
        images.append(img)
    _check(f"light-tracing {name}", images, reference, "box", "phong5:light" if name == "phong5" else name, also=lit)


# ---- ao
@pytest.mark.parametrize("limit", [1.0, None])
def test_ao_in_the_box(reference, limit):
    """The cosine-weighted open share of the hemisphere, nothing within `limit` (None: nothing at all)."""
    fp, names = reference.get("ao")
    value, error = (v[names.index(str(limit))] for v in fp.mean())
    ctx = _context(scenes.cbox(W, H))
    images = [ctx.render_ao(_seeds(k), spp=SPP_AO, max_distance=limit)[0] for k in range(K)]
    Q.check_ratios(f"ao box max_distance {limit}", [img.mean(axis=(0, 1)) / value for img in images], error / value)


@pytest.mark.parametrize("case", AO_BACK_CASES)
def test_ao_on_the_back_of_a_light(reference, case):
    """normal_correction where it acts: open_floor(light_in_view=True) shows the camera the back of the light's quad, the one surface that is not turned
    towards the viewer.  Without the flag those pixels are black (asserted); with it the hemisphere is the one on the viewer's side, open but for the canopy.
    A hemisphere left on the emitting side would see the floor 1.5 below: black with no limit, partly open at max_distance = 2.  With the flag the pixels
    of the back alone are held too: they are a fifth of the frame, and the floor around them would dilute a fault five-fold."""
    fp, names = reference.get("ao_back")
    sd = open_floor(W, H, light_in_view=True)
    sc = orc.Scene(sd)
    o, d = (np.asarray(a) for a in zip(*[sc.camera_generate(x + 0.5, y + 0.5) for y in range(H) for x in range(W)]))
    back = (sc.trace(o, d)[3] == 2).reshape(H, W) & (fp._pix["2n", 2][names.index(str(AO_BACK_CASES[0]))][..., 0] == 0.0)
    assert back.sum() >= 20, "the light's back fills too few pixels"
    ctx = _context(sd)
    images = [ctx.render_ao(_seeds(k), spp=64, max_distance=case[0], normal_correction=case[1])[0] for k in range(K)]
    _check(f"ao back of a light {case}", images, reference, "ao_back", str(case))
    if case[1]:
        _check(f"ao back of a light {case}, the back's pixels", images, reference, "ao_back", str(case), also=back)
    else:
        assert not any(img[back].any() for img in images)


@pytest.mark.parametrize("limit", [1.5, None])
def test_ao_on_the_open_floor(reference, limit):
    """The floor under the occluder (1 above it) and the light's quad (2 above): with max_distance = 1.5 the light's quad is out of reach everywhere and the
    occluder within reach of the floor beneath it; tests/test_surface_quadrature.py holds this quadrature to the form factor's closed form."""
    fp, names = reference.get("ao_floor")
    value, error = (v[names.index(str(limit))] for v in fp.mean())
    ctx = _context(open_floor(W, H))
    images = [ctx.render_ao(_seeds(k), spp=64, max_distance=limit)[0] for k in range(K)]
    Q.check_ratios(f"ao floor max_distance {limit}", [img.mean(axis=(0, 1)) / value for img in images], error / value)


# ---- path, direct through delta surfaces: glass, the smooth metal, the smooth substrate
STRATEGY = {"all": api.STRATEGY_ALL, "bsdf": api.STRATEGY_BSDF, "emitter": api.STRATEGY_EMITTER}
FUSED, WAVEFRONT = (api.PIPELINE_FUSED, api.STREAM_PER_SAMPLE), (api.PIPELINE_WAVEFRONT, api.STREAM_PER_SAMPLE)


class _DeltaScenes:
    """Per scene of DELTA_SCENES the scene, its context (one streamed, where asked) and Q.delta_reference at the gate and at max_edges = 2, each made once."""

    def __init__(self):
        self._made = {}

    def _once(self, key, make):
        if key not in self._made:
            self._made[key] = make()
        return self._made[key]

    def sd(self, scene):
        return self._once(("sd", scene), lambda: DELTA_SCENES[scene][0](W, H))

    def context(self, scene, streaming=False):
        return self._once(("context", scene, streaming), lambda: _context(self.sd(scene), streaming=streaming))

    def reference(self, scene, max_edges=None):
        def make():
            sd = self.sd(scene)
            strategies = ("all", "bsdf", "emitter") if scene == "pane" else ("all", "emitter")
            made = Q.delta_reference(orc.Scene(sd), sd, max_edges or DELTA_SCENES[scene][1], strategies, n=DELTA_SCENES[scene][2])
            assert made[0].keep.mean() >= 0.9, "more than 10 % of the pixels masked"
            print(f"reference {scene} to {max_edges or DELTA_SCENES[scene][1]} edges: {int((~made[0].keep).sum())} of {W * H} pixels masked")
            return made
        return self._once(("reference", scene, max_edges or DELTA_SCENES[scene][1]), make)

    def path(self, scene, strategy, pipeline, stream_mode, streaming=False, below=0, **kw):
        params = dict(max_depth=DELTA_SCENES[scene][1] + 1 - below, strategy=STRATEGY[strategy], pipeline=pipeline, stream_mode=stream_mode, **kw)
        ctx = self.context(scene, streaming)
        return [ctx.render(_seeds(k), api.path_params(Q.DELTA_SPP, **params))[0] for k in range(K)]


@pytest.fixture(scope="module")
def delta(built):
    return _DeltaScenes()


@pytest.mark.parametrize("pipeline,stream_mode", [FUSED, WAVEFRONT])
@pytest.mark.parametrize("strategy", ["all", "emitter"])
@pytest.mark.parametrize("scene", [s for s in DELTA_SCENES if s != "coat"])
def test_path_through_delta_surfaces(delta, scene, strategy, pipeline, stream_mode):
    """path at the scene's gate, max_depth = max_edges + 1 (confirmed on the CPU oracle, tests/test_surface_quadrature.py), against Q.delta_radiance: the
    dielectric Fresnel term and Snell's direction on both sides of a pane and of the critical angle, the choice between the two branches and its weight, the
    smooth metal's Fresnel factor, the MIS weight of a discrete edge, and under "emitter" the edge that left a delta vertex counting for nothing."""
    images = delta.path(scene, strategy, pipeline, stream_mode)
    if strategy == "all" and scene != "mirror_light":
        fp, _ = delta.reference(scene)
        below = delta.path(scene, strategy, pipeline, stream_mode, below=1)
        assert np.all(np.mean([img[fp.keep].mean(axis=0) for img in below], axis=0) < np.mean([img[fp.keep].mean(axis=0) for img in images], axis=0))
    Q.check_footprint(f"path {scene} {strategy} pipeline {pipeline}", images, delta.reference(scene), strategy)


@pytest.mark.parametrize("pipeline,stream_mode", [FUSED, WAVEFRONT])
def test_path_on_the_coat(delta, pipeline, stream_mode):
    """The smooth substrate: Schlick's F along the mirror direction beside the diffuse term, each sampled half the time.  One below the gate the frame is
    black, and under "emitter" it is black at the gate too: no light sample is made at a smooth vertex (surface_quadrature's smooth_substrate_nee)."""
    fp, _ = delta.reference("coat")
    assert not any(img[fp.keep].any() for img in delta.path("coat", "all", pipeline, stream_mode, below=1))
    assert not any(img.any() for img in delta.path("coat", "emitter", pipeline, stream_mode))
    Q.check_footprint(f"path coat all pipeline {pipeline}", delta.path("coat", "all", pipeline, stream_mode), delta.reference("coat"), "all")


@pytest.mark.parametrize("how", ["bsdf", "reference_order", "stratified", "streaming"])
def test_path_through_the_pane_the_other_ways(delta, how):
    """The pane from outside under the "bsdf" strategy, the reference-order streams, `-r stratified` and the streamed scene, once each."""
    kw = {"bsdf": dict(stream_mode=api.STREAM_PER_SAMPLE), "reference_order": dict(stream_mode=api.STREAM_REFERENCE_ORDER),
          "stratified": dict(stream_mode=api.STREAM_STRATIFIED), "streaming": dict(stream_mode=api.STREAM_PER_SAMPLE, streaming=True)}[how]
    strategy = "bsdf" if how == "bsdf" else "all"
    Q.check_footprint(f"path pane {strategy} {how}", delta.path("pane", strategy, api.PIPELINE_AUTO, **kw), delta.reference("pane"), strategy)


@pytest.mark.parametrize("scene,nb,miss", [("mirror", (1, 1), False), ("mirror_light", (1, 1), False), ("coat", (1, 0), False), ("coat", (1, 1), True)])
def test_direct_at_a_delta_hit(delta, scene, nb, miss):
    """direct samples one direction at the first hit and looks for a light or the sky at its end: the delta tree at max_edges = 2.  At a smooth vertex it
    makes no light sample (direct.rs:76) and still weights a sampled direction of the substrate's diffuse half against one (direct.rs:148-169): with
    nb_light_samples > 0 the coat reads 0.64, 0.68, 0.73 on the CPU, the reference's own text, asserted to miss."""
    images = _direct(delta.context(scene), nb, 128)
    Q.check_footprint(f"direct {scene} {nb}", images, delta.reference(scene, 2), "all", expect_miss=miss)


def test_zero_variance_in_the_mirror(delta):
    """The pixels every footprint ray of which ends on the light by way of the mirror, without russian roulette: every seed's pixel is the footprint mean of
    specular F Le under "all" and "bsdf" (a discrete edge has MIS weight 1), within Q.mirror_pixel_bound, and exactly 0 under "emitter"."""
    sd = delta.sd("mirror_light")
    inside, value, spread = Q.light_in_a_mirror(orc.Scene(sd), sd)
    assert inside.sum() >= 2, "the light's image fills too few pixels"
    bound = Q.mirror_pixel_bound(value, spread, Q.DELTA_SPP)[inside]
    for pipeline, stream_mode in (FUSED, WAVEFRONT):
        for strategy in ("all", "bsdf"):
            for img in delta.path("mirror_light", strategy, pipeline, stream_mode, rr_depth=10):
                assert np.all(np.abs(img[inside] - value[inside]) <= bound), (strategy, pipeline, img[inside], value[inside], bound)
        assert not any(img[inside].any() for img in delta.path("mirror_light", "emitter", pipeline, stream_mode, rr_depth=10))


def test_path_finds_the_caustic_by_sampled_directions(delta):
    """The caustic under "bsdf": the one pure BSDF-sampling case that needs 512 spp to stay under SE 5 % (a sampled direction finds the light's image once in
    a thousand)."""
    ctx = delta.context("caustic")
    params = dict(max_depth=4, strategy=api.STRATEGY_BSDF, pipeline=api.PIPELINE_AUTO, stream_mode=api.STREAM_PER_SAMPLE)
    images = [ctx.render(_seeds(k), api.path_params(512, **params))[0] for k in range(K)]
    Q.check_footprint("path caustic bsdf", images, delta.reference("caustic"), "all")


def test_light_tracing_on_the_caustic(delta):
    """light -> mirror -> floor -> camera, the light kernel through a discrete vertex: max_depth = 3 holds direct lighting plus the image source, one below holds
    direct lighting alone (the tree's "emitter" frame), and against that frame the depth-3 image is asserted to miss."""
    ctx = delta.context("caustic")
    lit = np.zeros((H, W), bool)
    lit[:, :W - (W - H) // 2] = True
    for max_depth, name in ((2, "emitter"), (3, "all")):
        images = []
        for k in range(K):
            img, st = ctx.render_light(_seeds(k), spp=Q.LIGHT_CAUSTIC_SPP, max_depth=max_depth)
            assert st["splats_invalid"] == 0 and st["splats_saturated"] == 0 and not img[~lit].any()
            images.append(img)
        Q.check_footprint(f"light-tracing caustic max_depth {max_depth}", images, delta.reference("caustic"), name, also=lit)
    Q.check_footprint("light-tracing caustic max_depth 3, no image source", images, delta.reference("caustic"), "emitter", also=lit, expect_miss=True)


def test_both_transports_on_the_single_crossing(delta):
    """tests.scene_helpers.lit_through_a_pane, a floor lit through one pane of glass: `path` at max_depth = 4 holds glass_radiance_scale = "none" and misses
    "eta2", light-tracing at max_depth = 3 holds "eta2" and misses "none" (the reference's text: both walk under Transport::Importance, which is the
    published model for a light path and lacks eta^2 for a camera path).  One below either gate, and under "emitter", the frame is black."""
    sd = lit_through_a_pane(W, H)
    sc, ctx = orc.Scene(sd), _context(sd)
    none, eta2 = (Q.delta_reference(sc, sd, 3, ("all",), dict(Q.REFERENCE, glass_radiance_scale=scale)) for scale in ("none", "eta2"))
    assert none[0].keep.mean() >= 0.9, "more than 10 % of the pixels masked"
    params = dict(pipeline=api.PIPELINE_AUTO, stream_mode=api.STREAM_PER_SAMPLE)
    assert not ctx.render(_seeds(0), api.path_params(16, max_depth=4, strategy=api.STRATEGY_EMITTER, **params))[0].any()
    assert not ctx.render(_seeds(0), api.path_params(16, max_depth=3, strategy=api.STRATEGY_ALL, **params))[0].any()
    for strategy in ("all", "bsdf"):
        images = [ctx.render(_seeds(k), api.path_params(Q.CROSSING_SPP, max_depth=4, strategy=STRATEGY[strategy], **params))[0] for k in range(K)]
        Q.check_footprint(f"path through one pane {strategy}", images, none, "all")
        Q.check_footprint(f"path through one pane {strategy}, published scaling", images, eta2, "all", expect_miss=True)
    lit = np.zeros((H, W), bool)
    lit[:, :W - (W - H) // 2] = True
    assert not ctx.render_light(_seeds(0), spp=16, max_depth=2)[0].any()
    images = [ctx.render_light(_seeds(k), spp=Q.LIGHT_CAUSTIC_SPP, max_depth=3)[0] for k in range(K)]
    Q.check_footprint("light-tracing through one pane", images, eta2, "all", also=lit)
    Q.check_footprint("light-tracing through one pane, path's scaling", images, none, "all", also=lit, expect_miss=True)
