"""The beam half of a map — the sub-beams of its surface beams and the beam tree over them — is the same whichever map owns it: from one hand-made set of
surface-beam records, rl_beam_map_build_words, rl_vrl_map_build_words and rl_pplane_map_build_words (the last beside one hand-made plane) give boxes, links
and sub-beams that are equal byte for byte, and equal to the host-only rl_beam_split + rl_beam_tree_build.  Two sizes: one beam (5 or 6 sub-beams: a root
over two leaves) and 40 beams of mixed lengths (a tree with inner nodes below the root).  Every beam has word 7 bit 0 set, so the VRL partition keeps all."""
import numpy as np
import pytest

from rustlight_amd import api, scenes
from tests import beam_restatement as R
from tests.beam_half_cases import assert_beam_half
from tests.scene_helpers import context as _context
from tests.test_gpu_pplane_exact import _hand_made

pytestmark = pytest.mark.gpu

RADIUS, N_PATHS = 0.1, 7


def _beams(n):
    rs = np.random.RandomState(31 + n)
    d = rs.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    o = rs.uniform((-0.9, 0.1, -0.9), (0.9, 1.9, 0.9), (n, 3)).astype(np.float32)
    length = np.where(np.arange(n) % 4 == 0, rs.uniform(1.0, 2.5, n), rs.uniform(0.05, 0.6, n)).astype(np.float32)      # a few long beams among short ones
    return R.beam_words(o, length, d, rs.uniform(0.5, 4.0, (n, 3)), from_surface=True, path=np.arange(n) % N_PATHS)


@pytest.mark.parametrize("n_beams", [1, 40])
def test_the_beam_half_is_the_same_in_every_map(built, n_beams):
    sd = scenes.cbox_medium(40, 24, 1.0)
    ctx = _context(sd)
    words = _beams(n_beams)
    assert (words[:, 7] & 1).all()
    plane = _hand_made(sd)[2][:1]
    bmap = ctx.beam_map_from_words(words, N_PATHS, RADIUS)
    vmap = ctx.vrl_map_from_words(words, N_PATHS, RADIUS)
    pmap = ctx.pplane_map_from_words(words, plane, N_PATHS, RADIUS)
    halves = {"beam map": bmap.read(), "VRL map": vmap.read()[:3], "photon-plane map": pmap.read("beams")}
    sizes = {what: assert_beam_half(got, words, RADIUS, what) for what, got in halves.items()}
    n_sub, n_nodes = sizes["beam map"]
    if n_beams == 1:
        assert n_sub in (5, 6) and n_nodes == 3
    else:
        assert n_sub > 4 * n_beams and n_nodes > 7                    # about 5 sub-beams per beam: inner nodes below the root
    want = halves["beam map"]
    for what, got in halves.items():                                  # and to each other, bit for bit
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), what
    assert vmap.info()[:4] == (n_beams, n_sub, n_nodes, 0)            # every beam stayed a surface beam: no VRL
    assert bmap.info()[:3] == (n_beams, n_sub, n_nodes) and pmap.info()[:5] == (n_beams, n_sub, n_nodes, 1, 1)
