"""The uncorrelated photon planes on the device held to tests/volume_quadrature.py, the float64 single-scattering quadrature that shares no code with the
kernel or the restatement, in the frame of tests/test_gpu_volume_quadrature.py: 24 x 18 (2 x 2 blocks, both edges ragged), the Cornell box with its medium and
black walls, K = 8 seeds at 1 spp, volume_quadrature.check_ratios over r_k = mean(image_k) / mean(quadrature) with the quadrature along the very camera rays
of seed k (at most 10 % of the pixels masked, asserted) times the case's factor: SE(r) <= 5 % and |mean(r) - 1| <= 4 SE(r) + the quadrature's error.

The rays are this integrator's: lane c of a block draws its jitter at c D and c D + 1 of the block's stream, D = 2 + NB * 7 (uv, vt, ut, ualpha, cmis) or
2 + NB * 8 (average, discrete_mis), 2 draws later for every direction drawn again before it.  At NB planes a frame takes 5 * 10^7 draws and about every
second frame draws a direction again, so tests/uplane_restatement.camera_rays finds the redraws from the streams' exact zeros, and every render's redraw
counter is held to the count the rays were made with.

The factor is 1 for uv, vt, ut, ualpha and cmis and 1 / 3 for average and discrete_mis — the reference's kept behaviour: they pick ONE of three plane types with
probability 1 / 3, weight it by 1 / 3 (or by a balance weight that sums to 1 over the types) and still divide by nb_primitive.  In the coloured medium uv
carries plane-single's kept bias sigma_t / sigma_s through the shared plane_new (tests/test_gpu_volume_quadrature.py has why).

NB = 2^14 planes per camera sample: the restatement's single-image spread on the CPU at 2048 planes x 768 rays was 1.7 % (ut) to 9 % (cmis) of the mean; at
2^14 x 432 that is at most 4.2 % per image and 1.5 % over K = 8.  What each case reaches on the device is in profiles/volume_quadrature_note.md."""
import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import uplane_restatement as U
from tests import volume_quadrature as Q
from tests.scene_helpers import add_second_light, black_walls, context as _context

pytestmark = pytest.mark.gpu

W, H, K = 24, 18, 8
CAM_SEED = 2000                                      # seed k looks through the block seeds of CAM_SEED + k
NB = 1 << 14
MEDIA = {                                            # name: (sigma_s, sigma_a)
    "grey": ((1.0,) * 3, (0.0,) * 3),
    "coloured": ((0.4, 1.0, 1.5), (1.2, 0.6, 0.1)),  # sigma_t = 1.6 in every channel, sigma_s / sigma_t = 0.25, 0.625, 0.9375
}
NAMES = ["grey", "coloured"]


def _scene(medium, second_light=False):
    ss, sa = MEDIA[medium]
    sd = scenes.cbox(W, H, scenes.Medium(sa, ss, scenes.PHASE_ISOTROPIC, 0.0))
    if second_light:
        add_second_light(sd)
    return black_walls(sd)


def _triple(medium):
    ss, sa = MEDIA[medium]
    return np.asarray(ss), np.asarray(ss) + np.asarray(sa), None


class _Reference:
    """The quadratures along the rays of every seed, per scene and plane layout, each computed once and left unchanged."""

    def __init__(self):
        self._along, self._zeros = {}, {}

    def cam_seeds(self, k):
        return orc.block_seeds(CAM_SEED + k, W, H)

    def _zeros_of(self, seed, variant, n):
        """A block stream's exact zeros, found once: over the longer layout's reach when the shorter one asks first."""
        reach = n // U.draws_per_sample(NB, "ut") * U.draws_per_sample(NB, "average")
        if (seed, variant) not in self._zeros or self._zeros[(seed, variant)][0] < n:
            self._zeros[(seed, variant)] = (reach, U.zero_draws(seed, variant, reach))
        z = self._zeros[(seed, variant)][1]
        return z[z < n]

    def along_rays(self, which, strategy):
        """[K] of {"px", "py", "keep", "redraws", "value": {name: [3]}, "error": {name: [3]}} for the plane layout of `strategy`."""
        key = (which, U.draws_per_plane(strategy))
        if key not in self._along:
            sd = _scene("grey", second_light=which == "two_lights")
            sc = orc.Scene(sd)
            out = []
            for k in range(K):
                px, py, o, d, tfar, redraws = U.camera_rays(sc, sd, self.cam_seeds(k), NB, strategy, zeros_of=self._zeros_of)
                keep = ~Q.near_a_light(sd, o, d, tfar, Q.NEAR)
                assert keep.mean() >= 0.9, "more than 10 % of the pixels masked"
                value, error = Q.image_mean(sc, sd, o, d, tfar, keep, media=[_triple(n) for n in NAMES])
                out.append({"px": px, "py": py, "keep": keep, "redraws": redraws, "value": dict(zip(NAMES, value)), "error": dict(zip(NAMES, error))})
            self._along[key] = out
        return self._along[key]


@pytest.fixture(scope="module")
def reference(built):
    return _Reference()


def _check(label, sd, strategy, reference, which, medium, factor=1.0):
    refs = reference.along_rays(which, strategy)
    ctx = _context(sd)
    rs = []
    for k, ref in enumerate(refs):
        img, st = ctx.render_plane_uncorrelated(reference.cam_seeds(k), NB, strategy, 1)
        assert st["redraws"] == ref["redraws"], (k, st["redraws"], ref["redraws"])          # the rays of the quadrature are the kernel's
        rs.append(img[ref["py"], ref["px"]][ref["keep"]].mean(axis=0) / (factor * ref["value"][medium]))      # relative to what is expected: SE and margin are fractions of it
    err = np.max([ref["error"][medium] / ref["value"][medium] for ref in refs], axis=0)
    return Q.check_ratios(label, rs, err)


@pytest.mark.parametrize("strategy", api.PLANE_STRATEGIES)
def test_uplane_in_the_grey_medium(reference, strategy):
    """Isotropic, sigma_s = 1: 1 / (4 pi), 1 / nb_primitive, every strategy's weight; a third of the radiance under average and discrete_mis, kept."""
    factor = 1.0 / 3.0 if strategy in ("average", "discrete_mis") else 1.0
    _check(f"uplane {strategy} grey", _scene("grey"), strategy, reference, "box", "grey", factor)


@pytest.mark.parametrize("strategy", ["ut", "uv"])
def test_uplane_in_the_coloured_medium(reference, strategy):
    """sigma_s = (0.4, 1.0, 1.5) with sigma_a = (1.2, 0.6, 0.1): sigma_s where sigma_t belongs is off by a different factor in every channel.  uv carries
    plane_new's pi Le / sigma_s where the free path's density asks for pi Le / sigma_t: sigma_t / sigma_s = (4, 1.6, 1.0667) times the radiance, kept."""
    ss, sa = MEDIA["coloured"]
    factor = (np.asarray(ss) + np.asarray(sa)) / np.asarray(ss) if strategy == "uv" else 1.0
    _check(f"uplane {strategy} coloured", _scene("coloured"), strategy, reference, "box", "coloured", factor)


def test_uplane_with_two_lights(reference, strategy="ut"):
    """n_lights and id_emitter: the second light emits (4, 6, 9) where the first emits (17, 12, 4), so a wrong share shows per channel."""
    sd = _scene("grey", second_light=True)
    assert len(Q.lights_of(sd)) == 2
    _check(f"uplane {strategy} two lights", sd, strategy, reference, "two_lights", "grey")
