"""The five volume integrators on the device held to tests/volume_quadrature.py, the float64 single-scattering quadrature that shares no code with the
kernels, the oracle's shading or the restatements (tests/test_volume_quadrature.py holds the quadrature itself to closed forms).  A term that kernel and
restatement both read wrongly from the reference's text (a missing sigma_s, 1 / (4 pi), 1 / number_plane_gen, CMIS's 2 / pi, Average's 1 / 3, the beam
estimate's 1 / (pi r^2), n_lights, the phase function's argument) passes every bit-exact test and fails here.

Frame 24 x 18 (2 x 2 blocks, both edges ragged), the Cornell box with its medium and black, non-emissive walls, so that nothing continues past a surface.
The statistic is volume_quadrature.check_ratios over K = 8 seeds: r_k = mean(image_k) / mean(quadrature), one ratio per seed and channel, over the pixels
whose rays stay NEAR away from every light (at most 10 % masked, asserted); asserted SE(r) <= 5 % and |mean(r) - 1| <= 4 SE(r) + the quadrature's error.

  plane-single, bre: 1 spp, and the quadrature runs along the very camera rays of seed k (bre_restatement.camera_samples with the block seeds the render is
      given): a few pixels near the light carry the mean, so the rays must be shared.
  path, light-tracing, vpl: so many samples per pixel that the jitter averages out; the reference is volume_quadrature.Footprint.

Depth gates that leave camera -> medium vertex -> light alone (each confirmed on the CPU oracle against the quadrature, profiles/volume_quadrature_note.md):
  bre             photons of rl_vpl_generate(VPL_VOLUME, max_depth = 2): a light path walks its light vertex only and stores its first medium vertex
                  (records <= paths and vertices == paths, asserted);
  path            max_depth = 3, min_depth = 1, strategy = emitter (max_depth = 2 is black);
  light-tracing   max_depth = 2 (max_depth = 1 is black); the box carries scene_helpers.with_back_triangle, because a connection to the camera that misses
                  the scene's root box counts as occluded (the reference's BVH, as in test_light_agrees_with_path).  On a frame wider than high the reference's
                  Camera::importance (camera.rs:130, `p.x > image_rect_max.y`) gives no importance to the last (W - H) / 2 columns: they are black, asserted,
                  and left out of the comparison;
  vpl             the emitter VPLs of rl_vpl_generate(VPL_SURFACE, max_depth = 2) gathered at the camera ray's medium vertex (option_lt = VPL_VOLUME); the
                  volume VPLs are scattering events themselves and would add double scattering.  The reference gathers nothing on a camera ray that
                  leaves the scene, so those rays are black in this one reference (Footprint.mean(dark=True)).

The counts are constants chosen for SE <= 2 % from the spread the restatements and the oracle show on the CPU; what each case reaches on the device is in
profiles/volume_quadrature_note.md."""
import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import bre_restatement as B
from tests import volume_quadrature as Q
from tests.scene_helpers import add_second_light, black_walls, context as _context, with_back_triangle

pytestmark = pytest.mark.gpu

W, H, K = 24, 18, 8
GEN_SEED, CAM_SEED = 1000, 2000                      # seed k generates with GEN_SEED + k and looks through the block seeds of CAM_SEED + k
NB_PLANES = 1 << 16
NB_PHOTONS = 1 << 15                                 # per-path streams; at sigma_s = 0.025 4.7 paths store one photon, and RL_VPL_MAX_PATHS is 2^18
NB_PHOTONS_SERIAL = 1 << 13                          # the serial stream walks one path at a time
NB_VPL, SPP_VPL = 4096, 16
SPP_PATH = SPP_LIGHT = 1024
G, G_PLANE = 0.6, -0.8
MEDIA = {                                            # name: (sigma_s, sigma_a, g)
    "grey": ((1.0,) * 3, (0.0,) * 3, None),
    "grey_hg": ((1.0,) * 3, (0.0,) * 3, G_PLANE),
    "coloured": ((0.4, 1.0, 1.5), (1.2, 0.6, 0.1), None),            # sigma_t = 1.6 in every channel, sigma_s / sigma_t = 0.25, 0.625, 0.9375
    "chromatic": ((0.5, 0.75, 1.0), (0.0,) * 3, None),                # sigma_t differs per channel
    "thin": ((0.025,) * 3, (0.0,) * 3, None),
    "thin_hg": ((0.025,) * 3, (0.0,) * 3, G),
    "sparse": ((0.05,) * 3, (0.0,) * 3, None),                        # path, light-tracing, vpl: at sigma_s = 1 the 5.8 units before the box leave e^-6
    "sparse_hg": ((0.05,) * 3, (0.0,) * 3, G),
}


def _scene(medium, second_light=False, back_triangle=False):
    ss, sa, g = MEDIA[medium]
    sd = scenes.cbox(W, H, scenes.Medium(sa, ss, scenes.PHASE_ISOTROPIC if g is None else scenes.PHASE_HG, 0.0 if g is None else g))
    if second_light:
        add_second_light(sd)
    if back_triangle:
        with_back_triangle(sd)
    return black_walls(sd)


def _triple(medium, g="own"):
    ss, sa, own = MEDIA[medium]
    return np.asarray(ss), np.asarray(ss) + np.asarray(sa), (own if g == "own" else g)


class _Reference:
    """The quadratures, each computed once and left unchanged: per seed along the seed's camera rays, and over the pixel footprints."""
    ALONG_RAYS = {"box": ["grey", "grey_hg", "coloured", "chromatic", "thin", "thin_hg"], "two_lights": ["grey"]}

    def __init__(self):
        self._rays, self._footprint = {}, None

    def cam_seeds(self, k):
        return orc.block_seeds(CAM_SEED + k, W, H)

    def along_rays(self, which):
        """[K] of {"px", "py", "keep", "value": {name: [3]}, "error": {name: [3]}}; the box adds "chromatic:channel_mean" (volume_quadrature.radiance's
        free_path)."""
        if which not in self._rays:
            sd = _scene("grey", second_light=which == "two_lights")
            sc = orc.Scene(sd)
            names = self.ALONG_RAYS[which]
            media = [_triple(n) for n in names]
            out = []
            for k in range(K):
                px, py, o, d, tfar = B.camera_samples(sc, sd, self.cam_seeds(k), 1)
                keep = ~Q.near_a_light(sd, o, d, tfar, Q.NEAR)
                assert keep.mean() >= 0.9, "more than 10 % of the pixels masked"
                value, error = Q.image_mean(sc, sd, o, d, tfar, keep, media=media)
                out.append({"px": px, "py": py, "keep": keep, "value": dict(zip(names, value)), "error": dict(zip(names, error))})
                if which == "box":
                    value, error = Q.image_mean(sc, sd, o, d, tfar, keep, media=[_triple("chromatic")], free_path="channel_mean")
                    out[-1]["value"]["chromatic:channel_mean"], out[-1]["error"]["chromatic:channel_mean"] = value[0], error[0]
            self._rays[which] = out
        return self._rays[which]

    def footprint(self):
        """(the volume_quadrature.Footprint of the box with the triangle behind the camera, the names of its media in order)."""
        if self._footprint is None:
            sd = _scene("sparse", back_triangle=True)
            names = ["sparse", "sparse_hg"]
            self._footprint = (Q.Footprint(orc.Scene(sd), sd, 2, Q.NEAR, media=[_triple(n) for n in names]), names)
            assert self._footprint[0].keep.mean() >= 0.9, "more than 10 % of the pixels masked"
        return self._footprint


@pytest.fixture(scope="module")
def reference(built):
    return _Reference()


def _check_along_rays(label, images, refs, medium, expect_medium=None, factor=1.0):
    """images[k] rendered at 1 spp through cam_seeds(k), against `factor` [3] times the quadrature of `expect_medium` (default: the medium itself)."""
    name = expect_medium or medium
    rs = [img[ref["py"], ref["px"]][ref["keep"]].mean(axis=0) / (factor * ref["value"][name]) for img, ref in zip(images, refs)]
    err = np.max([ref["error"][name] / ref["value"][name] for ref in refs], axis=0)
    return rs, Q.check_ratios(label, rs, err)


# ---- plane-single
def _plane_images(sd, strategy, reference):
    ctx = _context(sd)
    images = []
    for k in range(K):
        planes, _ = ctx.plane_generate(api.IndependentSampler(GEN_SEED + k), NB_PLANES, strategy)
        images.append(ctx.render_plane_single(ctx.plane_map(planes), reference.cam_seeds(k), 1)[0])
    return images


@pytest.mark.parametrize("strategy", api.PLANE_STRATEGIES)
def test_plane_single_in_the_grey_medium(reference, strategy):
    """Isotropic, sigma_s = 1: 1 / (4 pi), 1 / number_plane_gen, every strategy's weight (Average's 1 / 3, CMIS's 2 / pi, DiscreteMIS's sum)."""
    _check_along_rays(f"plane-single {strategy} grey", _plane_images(_scene("grey"), strategy, reference), reference.along_rays("box"), "grey")


@pytest.mark.parametrize("strategy", ["uv", "ut", "average", "cmis"])
def test_plane_single_in_the_coloured_medium(reference, strategy):
    """sigma_s = (0.4, 1.0, 1.5) with sigma_a = (1.2, 0.6, 0.1): sigma_s where sigma_t belongs, or a dropped sigma_s, is off by a different factor in every
    channel (sigma_s / sigma_t = 0.25, 0.625, 0.9375), while sigma_t = 1.6 is one number (the next test has why).

    A UV plane is the reference's own bias under absorption, kept and pinned: its weight is pi Le / sigma_s (plane_single.rs:199) where the density of the
    sampled free path, sigma_t e^{-sigma_t t}, asks for pi Le / sigma_t, so a UV plane's image is sigma_t / sigma_s = (4, 1.6, 1.0667) times the radiance;
    Average carries a third of that, (2 + sigma_t / sigma_s) / 3.  DiscreteMIS weights the UV plane by a function of the ray, so its bias under absorption
    is no constant factor: it is held in the grey medium and with two lights, not here."""
    ss, sa, _ = MEDIA["coloured"]
    uv = (np.asarray(ss) + np.asarray(sa)) / np.asarray(ss)
    factor = {"uv": uv, "average": (2.0 + uv) / 3.0}.get(strategy, 1.0)
    _check_along_rays(f"plane-single {strategy} coloured", _plane_images(_scene("coloured"), strategy, reference), reference.along_rays("box"), "coloured",
                      factor=factor)


def test_plane_single_mixes_the_channels_free_paths(reference):
    """The reference's own bias in a medium whose sigma_t differs between the channels, kept and pinned.  The plane pass takes a plane's extent from
    HomogenousVolume::sample's continued_t (plane_single.rs:347-357), the free path of one channel drawn at random, and drops the continued_w that would
    correct each channel for that choice: every channel sees the light through the mean of the three transmittances.  At sigma_t = (0.5, 0.75, 1.0) the ut
    image equals the quadrature with exactly that departure (free_path = "channel_mean") and misses the physical one by more than the margin in the outer
    channels."""
    refs = reference.along_rays("box")
    images = _plane_images(_scene("chromatic"), "ut", reference)
    _, (_, _, margin) = _check_along_rays("plane-single ut chromatic, channel-mean quadrature", images, refs, "chromatic", "chromatic:channel_mean")
    physical = np.mean([img[ref["py"], ref["px"]][ref["keep"]].mean(axis=0) / ref["value"]["chromatic"] for img, ref in zip(images, refs)], axis=0)
    print(f"plane-single ut chromatic, physical quadrature: r = {physical}")
    assert abs(physical[0] - 1.0) > margin[0] and abs(physical[2] - 1.0) > margin[2], (physical, margin)


@pytest.mark.parametrize("strategy", ["ut", "discrete_mis"])
def test_plane_single_with_two_lights(reference, strategy):
    """n_lights and id_emitter: the second light emits (4, 6, 9) where the first emits (17, 12, 4), so a wrong share shows per channel."""
    sd = _scene("grey", second_light=True)
    assert len(Q.lights_of(sd)) == 2
    _check_along_rays(f"plane-single {strategy} two lights", _plane_images(sd, strategy, reference), reference.along_rays("two_lights"), "grey")


def test_plane_single_ignores_the_phase_function(reference, strategy="ut"):
    """The kept quirk rho = Isotropic (plane_single.rs:440): in a Henyey-Greenstein medium of g = -0.8 the image equals the isotropic quadrature, and is
    further from the HG one than ten margins (the two quadratures differ five-fold there: test_the_phase_functions_are_told_apart)."""
    refs = reference.along_rays("box")
    images = _plane_images(_scene("grey_hg"), strategy, reference)
    rs, (_, _, margin) = _check_along_rays(f"plane-single {strategy} HG medium, isotropic quadrature", images, refs, "grey_hg", expect_medium="grey")
    apart = np.mean([ref["value"]["grey"] / ref["value"]["grey_hg"] for ref in refs], axis=0)
    assert np.all(np.abs(apart - 1.0) > 10.0 * margin), (apart, margin)
    against_hg = np.mean([img[ref["py"], ref["px"]][ref["keep"]].mean(axis=0) / ref["value"]["grey_hg"] for img, ref in zip(images, refs)], axis=0)
    print(f"plane-single {strategy} HG medium, HG quadrature: r = {against_hg}")
    assert np.all(np.abs(against_hg - 1.0) > margin), (against_hg, margin)


# ---- the beam radiance estimate
@pytest.mark.parametrize("medium,streams,nb", [("thin", "per_path", NB_PHOTONS), ("thin_hg", "per_path", NB_PHOTONS), ("grey", "reference", NB_PHOTONS_SERIAL),
                                               ("thin_hg", "reference", NB_PHOTONS_SERIAL)])
def test_bre(reference, medium, streams, nb):
    """First-scatter photons (max_depth = 2) of either stream kind, the tree built on the host and on the device: the same map, so the same image, asserted.
    g enters through phase(-d, d_in).  Radius 0.05: tests/test_volume_quadrature.py bounds its bias below 0.5 %."""
    ctx = _context(_scene(medium))
    images = []
    for k in range(K):
        vpls, st = ctx.vpl_generate(api.IndependentSampler(GEN_SEED + k), nb, max_depth=2, option_vpl=api.VPL_VOLUME, streams=streams)
        n, n_paths = vpls.info()[:2]
        assert nb <= n <= n_paths, (n, n_paths)                       # a path stores at most its first medium vertex
        if streams == "reference":
            assert st["vertices"] == n_paths
        by_build = [ctx.render_bre(ctx.photon_map(vpls, Q.BRE_RADIUS, build), reference.cam_seeds(k), 1)[0] for build in api.TREE_BUILDS]
        np.testing.assert_array_equal(by_build[0], by_build[1])
        images.append(by_build[0])
    _check_along_rays(f"bre {medium} {streams} {nb} photons", images, reference.along_rays("box"), medium)


# ---- path, light-tracing, vpl
def _check_footprint(label, images, reference, medium, dark=False, also=None):
    fp, names = reference.footprint()
    value, error = (v[names.index(medium)] for v in fp.mean(dark, also))
    keep = fp.keep if also is None else fp.keep & also
    return Q.check_ratios(label, [img[keep].mean(axis=0) / value for img in images], error / value)


@pytest.mark.parametrize("medium", ["sparse", "sparse_hg"])
def test_path(reference, medium):
    ctx = _context(_scene(medium, back_triangle=True))
    gate = dict(min_depth=1, strategy=api.STRATEGY_EMITTER)
    assert not ctx.render(reference.cam_seeds(0), api.path_params(4, max_depth=2, **gate))[0].any()
    images = [ctx.render(reference.cam_seeds(k), api.path_params(SPP_PATH, max_depth=3, **gate))[0] for k in range(K)]
    _check_footprint(f"path {medium}", images, reference, medium)


@pytest.mark.parametrize("strategy", [api.LIGHT_VOLUME, api.LIGHT_ALL])
@pytest.mark.parametrize("medium", ["sparse", "sparse_hg"])
def test_light_tracing(reference, medium, strategy):
    ctx = _context(_scene(medium, back_triangle=True))
    assert not ctx.render_light(reference.cam_seeds(0), spp=4, max_depth=1, strategy=strategy)[0].any()
    images = [ctx.render_light(reference.cam_seeds(k), spp=SPP_LIGHT, max_depth=2, strategy=strategy)[0] for k in range(K)]
    lit = np.zeros((H, W), bool)
    lit[:, :W - (W - H) // 2] = True                                  # Camera::importance's `p.x > image_rect_max.y`: columns 21 .. 23 get none
    for img in images:
        assert not img[~lit].any() and img[:, :(W - H) // 2].any()
    _check_footprint(f"light-tracing {medium} strategy {strategy}", images, reference, medium, also=lit)


@pytest.mark.parametrize("medium", ["sparse", "sparse_hg"])
def test_vpl(reference, medium):
    ctx = _context(_scene(medium, back_triangle=True))
    images = []
    for k in range(K):
        vpls, _ = ctx.vpl_generate(api.IndependentSampler(GEN_SEED + k), NB_VPL, max_depth=2, option_vpl=api.VPL_SURFACE)
        assert not (vpls.records()["kind"] == 1).any()                # RL_VPL_KIND_VOLUME: none, they would scatter a second time
        images.append(ctx.render_vpl(vpls, reference.cam_seeds(k), spp=SPP_VPL, option_lt=api.VPL_VOLUME)[0])
    _check_footprint(f"vpl {medium}", images, reference, medium, dark=True)
