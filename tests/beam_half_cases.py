"""Shared by the tests of the three maps that hold a beam half (BeamMap, VrlMap, PPlaneMap): the half read back from a map against the host-only split and
beam tree over the same surface-beam records."""
import numpy as np

from rustlight_amd import api
from tests.photon_tree_cases import assert_trees_equal


def assert_beam_half(got, surface_words, radius, what="map"):
    """got: (boxes, links, sub-beams [n_sub, 12] f32, ...) as a map's read() gives them.  Boxes and links are those of api.beam_tree_build over
    api.beam_split(surface_words), the sub-beams that split in leaf order packed o, length | d, 0 | radiance, 0, all byte for byte.  Returns (sub-beams,
    tree nodes) of the host build for the caller's info() assert."""
    sub = api.beam_split(surface_words)
    boxes, links, order = api.beam_tree_build(sub, radius)
    assert_trees_equal(got[:2], (boxes, links), what)
    f = sub[order].view(np.float32)
    want = np.zeros((sub.shape[0], 12), np.float32)
    want[:, 0:4], want[:, 4:7], want[:, 8:11] = f[:, 0:4], f[:, 4:7], f[:, 8:11]
    np.testing.assert_array_equal(got[2].view(np.uint32), want.view(np.uint32))
    return sub.shape[0], boxes.shape[0]
