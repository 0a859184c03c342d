"""Resources of the device forms of plane-single's set-up, read from the code-object notes as tests/test_photon_tree_resources.py does: the plane
instantiations of the tree kernels (kernels/planetree.hip) and k_plane_generate_lanes neither spill nor have a private segment; the plane subtree finish keeps
its LDS under half of what a gfx950 workgroup may declare (160 KiB), so that two of its workgroups share a compute unit; and making the tree kernels generic
cost the photon instantiations nothing.  Then, on the CPU, that the plane families of tests/plane_tree_cases.py hold what the GPU tests use them for — box
coordinates that are -0 and box coordinates that are +0, and tied sort keys — and which zero the host's box union keeps."""
import numpy as np

from rustlight_amd import api, resources
from tests import plane_tree_cases as P

PLANE_KERNELS = ("k_plt_box", "k_plt_finish", "k_plt_iota", "k_plt_merge", "k_plt_permute", "k_plt_pre", "k_plt_sort", "k_pt_planes")
LDS_PER_WORKGROUP = 160 * 1024
# the photon instantiations before the kernels were made generic over the element: (VGPRs, SGPRs, static LDS bytes, waves per SIMD the registers allow)
PHOTON_BEFORE = {"k_pt_box": (18, 28, 96, 8), "k_pt_check": (7, 15, 0, 8), "k_pt_finish": (165, 97, 56832, 3), "k_pt_iota": (4, 10, 0, 8),
                 "k_pt_merge": (11, 24, 0, 8), "k_pt_permute": (6, 24, 0, 8), "k_pt_photons": (8, 14, 0, 8), "k_pt_sort": (29, 57, 16640, 8)}
SGPR_BLOCK = 16          # scalar registers are allocated in blocks of 16, and a wave's share of them does not limit the waves per SIMD on gfx950


def _clean(r):
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch_bytes_per_lane"] == 0, r


def test_plane_tree_kernels_keep_their_budget(built):
    rows = {r["kernel"]: r for r in resources.kernel_resources() if r["object"] == "planetree.hip.o"}
    assert tuple(sorted(rows)) == PLANE_KERNELS
    for r in rows.values():
        _clean(r)
        assert r["lds_static_bytes"] <= LDS_PER_WORKGROUP, r
    finish = rows["k_plt_finish"]
    group = api.PLANE_TREE_GROUP_PLANES
    assert finish["lds_static_bytes"] == 51 * group + (group // 32) * 6 * 8          # 9 staged floats, record index, key, place, axis per plane; the box rows
    assert finish["lds_static_bytes"] <= LDS_PER_WORKGROUP // 2
    assert finish["max_waves_per_simd_by_vgpr"] >= 2                                 # 4 waves per workgroup, one per SIMD: two workgroups per compute unit


def test_lane_parallel_generation_keeps_its_budget(built):
    rows = {r["kernel"]: r for r in resources.kernel_resources() if r["object"] == "plane_generate.hip.o"}
    assert tuple(sorted(rows)) == ("k_plane_generate", "k_plane_generate_lanes")
    _clean(rows["k_plane_generate_lanes"])                                           # the jump-ahead is in line: no call frame, no private segment
    assert rows["k_plane_generate_lanes"]["lds_static_bytes"] == 0


def test_photon_instantiations_are_no_worse_than_before(built):
    rows = {r["kernel"]: r for r in resources.kernel_resources() if r["object"] == "phototree.hip.o"}
    assert sorted(rows) == sorted(PHOTON_BEFORE)
    for name, (vgpr, sgpr, lds, waves) in PHOTON_BEFORE.items():
        r = rows[name]
        print(name, (r["vgpr"], r["sgpr"], r["lds_static_bytes"], r["max_waves_per_simd_by_vgpr"]), "before", (vgpr, sgpr, lds, waves))
        _clean(r)
        assert r["vgpr"] <= vgpr and r["agpr"] == 0 and r["lds_static_bytes"] <= lds and r["max_waves_per_simd_by_vgpr"] >= waves, r
        assert -(-r["sgpr"] // SGPR_BLOCK) <= -(-sgpr // SGPR_BLOCK), r


def test_the_families_hold_signed_zero_boxes_and_tied_keys(built):
    seen = {"lo-": 0, "lo+": 0, "hi-": 0, "hi+": 0}
    for n in (9, 17, 100, 300, api.PLANE_TREE_GROUP_PLANES + 1):
        words = P.planes("zeros", n)
        c = P.corners(words).view(np.uint32)
        for a in range(3):                                                           # on every axis some plane has a corner at -0 beside one at +0
            assert (((c[:, a] == P.NEG_ZERO).any(axis=1)) & ((c[:, a] == 0).any(axis=1))).any(), (n, a)
        boxes = api.plane_tree_build(words)[0].view(np.uint32)
        for key, part, bits in (("lo-", boxes[:, :3], P.NEG_ZERO), ("lo+", boxes[:, :3], 0), ("hi-", boxes[:, 3:], P.NEG_ZERO), ("hi+", boxes[:, 3:], 0)):
            seen[key] += int((part == bits).sum())
        if n >= 100:
            assert all(int((part == bits).sum()) > 0 for part in (boxes[:, :3], boxes[:, 3:]) for bits in (P.NEG_ZERO, 0)), n
    print(seen)
    assert all(v > 0 for v in seen.values()), seen
    for family in ("tied", "equal", "zeros"):
        mid = P.middles(P.planes(family, 300))
        assert all(len(np.unique(mid[:, a])) < 150 for a in range(3)), family        # most keys are tied on every axis
    for family in ("degenerate",):
        w = P.planes(family, 300)
        assert (w[::3, 9] == 0).all() and (w[1::3, 3:6] == w[1::3, 6:9]).all()


def test_the_level_model_equals_the_host_build(built):
    """The two facts the plane kernels rest on, on the CPU: the 64-bit minimum (value, last place, its sign) is the host's box, signed zeros included, in
    any order of arrival, and any sort by (ordered key of the middle, place) is the host's stable sort."""
    rng = np.random.default_rng(5)
    for family in P.FAMILIES:
        for n in (1, 4, 5, 9, 17, 100, 300):
            words = P.planes(family, n)
            want = api.plane_tree_build(words)
            P.assert_trees_equal(P.levels_build(words), want, f"{family} n={n}")
            P.assert_trees_equal(P.levels_build(words, rng), want, f"{family} n={n}, shuffled")


def test_the_host_union_keeps_the_last_zero(built):
    """What kernels/phototree.hip.h states about the host build and restates on 64-bit words: of zeros of different sign the box keeps the LAST one, among a
    plane's corners and then among the planes of a leaf in their order."""
    pz, nz = np.float32(0.0), np.float32(-0.0)

    def leaf_box(x_of_o):                                                            # planes without extent at (x, 1, 1): one leaf, its box on x
        n = len(x_of_o)
        o = np.ones((n, 3), np.float32)
        o[:, 0] = x_of_o
        d = np.full((n, 3), nz)                                                      # -0 * 0 = -0, and x + -0 = x for either zero: all four corners are o
        return api.plane_tree_build(P.records(o, d, d, np.zeros(n), np.zeros(n)))[0].view(np.uint32)[0, [0, 3]]

    assert list(leaf_box([pz, nz])) == [P.NEG_ZERO, P.NEG_ZERO]
    assert list(leaf_box([nz, pz])) == [0, 0]
    assert list(leaf_box([nz, pz, nz, pz])) == [0, 0]
    # within one plane: o = -0, d0 = +1 and d1 = -0 with both lengths 0 give the corners -0, -0 + 0 = +0, -0 + -0 = -0, +0 + -0 = +0: the last is +0
    one = P.records([[nz, 1, 1]], [[1, 0, 0]], [[nz, 0, 0]], [0.0], [0.0])
    assert list(P.corners(one).view(np.uint32)[0, 0]) == [P.NEG_ZERO, 0, P.NEG_ZERO, 0]
    assert list(api.plane_tree_build(one)[0].view(np.uint32)[0, [0, 3]]) == [0, 0]
    # with both directions -0 every corner is o itself: -0 stays -0 at both ends of the box
    assert list(api.plane_tree_build(P.records([[nz, 1, 1]], [[nz, 0, 0]], [[nz, 0, 0]], [0.0], [0.0]))[0].view(np.uint32)[0, [0, 3]]) == [P.NEG_ZERO, P.NEG_ZERO]
