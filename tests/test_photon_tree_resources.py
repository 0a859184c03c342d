"""Resources of the device build of the photon tree (kernels/phototree.hip.h), read from the code-object notes like tests/test_vpl_paths_resources.py does:
no kernel of the family spills or has a private segment, and each one's LDS is within what a workgroup may declare on gfx950 (160 KiB); the subtree finish
stays under half of that, so that two of its workgroups share a compute unit."""
from rustlight_amd import resources

KERNELS = ("k_pt_box", "k_pt_check", "k_pt_finish", "k_pt_iota", "k_pt_merge", "k_pt_permute", "k_pt_photons", "k_pt_sort")
LDS_PER_WORKGROUP = 160 * 1024


def test_every_photon_tree_kernel_keeps_its_budget(built):
    rows = {r["kernel"]: r for r in resources.kernel_resources() if r["object"] == "phototree.hip.o"}
    assert tuple(sorted(rows)) == KERNELS
    for r in rows.values():
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
        assert r["scratch_bytes_per_lane"] == 0, r
        assert r["lds_static_bytes"] <= LDS_PER_WORKGROUP, r
    assert rows["k_pt_finish"]["lds_static_bytes"] <= LDS_PER_WORKGROUP // 2
    assert rows["k_pt_finish"]["max_waves_per_simd_by_vgpr"] >= 2          # 4 waves per workgroup, one per SIMD: two workgroups per compute unit
