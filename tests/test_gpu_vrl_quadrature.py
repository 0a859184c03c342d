"""The virtual ray lights on the device held to tests/vrl_quadrature.py, the float64 pair integral that shares no code with the kernels or with
tests/vrl_restatement.py: a factor both read wrongly from the reference's text (a sigma_s, 1 / rr, inv_pdf, 1 / dist^2) passes every bit-exact test and fails
here — tests/test_vrl_quadrature.py shows on the CPU that leaving out each of the four breaks the very assertion made below.

The setting is that file's, imported unchanged: the black-walled box behind a 6 degree lens, 24 x 18 pixels at 1 spp along the rays the quadrature integrates,
two hand-made bright VRLs beside the shaft of rays with rr = 1 (400 black VRLs) or rr = 0.75 (148), K = 8 seeds, volume_quadrature.check_ratios: SE <= 5 % and
|mean(render / quadrature) - 1| <= 4 SE + the quadrature's convergence error.  What the device reaches is in profiles/vrl_note.md."""
import numpy as np
import pytest

from tests import test_vrl_quadrature as T
from tests import volume_quadrature as VQ
from tests.scene_helpers import context as _context

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", sorted(T.N_BLACK))
def test_virtual_ray_lights(built, case):
    ctx = _context(T.scene())
    accepted = []

    def render(words, seeds):
        img, st = ctx.render_vrl(ctx.vrl_map_from_words(words, T.N_PATHS, T.RADIUS), seeds, 1)
        accepted.append(st["vrl_accepted"])
        assert st["beams_accepted"] == 0            # the one surface beam is black and out of the way: the image is the VRLs'
        return img

    rs = T.ratios(render, case)
    assert min(accepted) > T.W * T.H
    VQ.check_ratios(f"virtual-ray-lights {case}", rs, T.quadrature_error())
