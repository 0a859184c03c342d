"""The photon beams on the device held to tests/volume_quadrature.py, the float64 single-scattering quadrature that shares no code with the kernels or with
tests/beam_restatement.py: a term both read wrongly from the reference's text (a missing sigma_s, 1 / (4 pi), the kernel's 0.5 / r, 1 / sin_theta, the
1 / nb_path_shot) passes every bit-exact test and fails here.

The setting is tests/test_gpu_volume_quadrature.py's for the beam radiance estimate, whose scenes, seeds and statistic are imported unchanged: the 24 x 18 box
with black walls, 1 spp along the very camera rays the quadrature integrates, K = 8 seeds, volume_quadrature.check_ratios (SE(r) <= 5 % and |mean(r) - 1| <=
4 SE(r) + the quadrature's error).  max_depth = 2 leaves camera -> medium -> light alone: a light path walks its light vertex only and stores the one beam
that leaves the light (beams == paths, all from_surface, asserted).  The beam carries the light's flux and ends where the path scattered or hit, so a camera
ray meets it with the probability of the free path reaching that far: the transmittance.  Radius volume_quadrature.BRE_RADIUS, as for bre.

Media: grey and coloured, whose sigma_t is one number in every channel.  The chromatic medium is left out: a beam ignores its own edge's weight, so channels
of different sigma_t see the channel-mean free path along the beam.

The counts are constants chosen on the CPU from the spread the restatement shows (its intersection and contribution evaluated for every beam and camera ray,
over beams rebuilt from the oracle's two-vertex light paths; the serial beams are the device's, path for path).  The spread is heavy-tailed in these media:
the camera stands 5.8 units in front of the box, a beam reaches its side of the box with probability e^-6 (grey) or e^-9 (coloured) and is then seen through
a transmittance near 1 by a whole row of pixels, so a few per cent of the radiance sit in events a run rarely holds: a run without one reads 0.90 - 0.97,
a small run that holds one reads 1.2 to 16, and an event weighs 1 / count.  mean +- SE of the ratio over the 8 seeds, per count (* keeps the rule):
    count              2^10          2^11          2^12          2^13          2^14          2^15           2^16           2^17
    grey per-path      1.04 +- .053  0.99 +- .025* 1.34 +- .36   1.14 +- .18   1.04 +- .087  1.010 +- .041* 1.016 +- .031* 1.004 +- .017*
    grey serial        1.08 +- .14   1.03 +- .083  0.98 +- .042* 2.89 +- 1.9   1.93 +- .96   1.47 +- .48    1.23 +- .24    1.13 +- .12
    coloured per-path  0.98 +- .085  0.95 +- .061  1.08 +- .17   1.01 +- .080  0.97 +- .041* 0.947 +- .017* 0.942 +- .011  0.944 +- .014*
    coloured serial    1.57 +- .71   1.25 +- .36   1.09 +- .16   1.06 +- .092  0.98 +- .053  0.969 +- .028* 0.959 +- .014* 1.001 +- .037*
The count is 2^15, test_bre's per-path count and the largest whose host tree builds leave a case at a few seconds, wherever the restatement keeps the rule
there: both per-path cases and the coloured serial one.  The grey serial stream holds, in its eighth seed, a beam before path 8192 that crosses the frustum
next to the camera and reads 16 at 2^13 beams and still 1.9 at 2^17: that case takes 2^12, the one count at which the restatement keeps the rule.  What each
case reaches on the device is in profiles/beam_note.md."""
import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api
from tests import bre_restatement as B
from tests import volume_quadrature as Q
from tests.scene_helpers import context as _context
from tests.test_gpu_volume_quadrature import CAM_SEED, GEN_SEED, H, K, W, _scene, _triple

pytestmark = pytest.mark.gpu

NB_BEAMS = 1 << 15
NB_BEAMS_GREY_SERIAL = 1 << 12
NAMES = ["grey", "coloured"]


@pytest.fixture(scope="module")
def reference(built):
    """[K] of {"seeds", "px", "py", "keep", "value": {name: [3]}, "error": {name: [3]}}: the quadrature along each seed's camera rays, computed once."""
    sd = _scene("grey")
    sc = orc.Scene(sd)
    out = []
    for k in range(K):
        seeds = orc.block_seeds(CAM_SEED + k, W, H)
        px, py, o, d, tfar = B.camera_samples(sc, sd, seeds, 1)
        keep = ~Q.near_a_light(sd, o, d, tfar, Q.NEAR)
        assert keep.mean() >= 0.9, "more than 10 % of the pixels masked"
        value, error = Q.image_mean(sc, sd, o, d, tfar, keep, media=[_triple(n) for n in NAMES])
        out.append({"seeds": seeds, "px": px, "py": py, "keep": keep, "value": dict(zip(NAMES, value)), "error": dict(zip(NAMES, error))})
    return out


@pytest.mark.parametrize("medium,streams,nb", [("grey", "per_path", NB_BEAMS), ("coloured", "per_path", NB_BEAMS), ("grey", "reference", NB_BEAMS_GREY_SERIAL),
                                               ("coloured", "reference", NB_BEAMS)])
def test_photon_beams(reference, medium, streams, nb):
    ctx = _context(_scene(medium))
    rs = []
    for k, ref in enumerate(reference):
        beams, st = ctx.beam_generate(api.IndependentSampler(GEN_SEED + k), nb, max_depth=2, streams=streams)
        n, n_paths = beams.info()
        assert n == n_paths == nb and st["vertices"] == n_paths           # one beam per path, from the light vertex
        assert (beams.words()[:, 7] == 1).all()
        img = ctx.render_beams(ctx.beam_map(beams, Q.BRE_RADIUS), ref["seeds"], 1)[0]
        rs.append(img[ref["py"], ref["px"]][ref["keep"]].mean(axis=0) / ref["value"][medium])
    err = np.max([ref["error"][medium] / ref["value"][medium] for ref in reference], axis=0)
    Q.check_ratios(f"photon-beams {medium} {streams} {nb} beams", rs, err)
