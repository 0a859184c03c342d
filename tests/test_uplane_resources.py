"""Register budgets of the uncorrelated photon-plane kernel (kernels/uplane.hip.h), read from the code-object notes like tests/test_plane_single_resources.py
does: every instantiation of k_uplane without VGPR spill and without a private segment, at three waves per SIMD or more — the bar k_plane_gather is held to.
rng_advance<false> keeps the jump table's step in line for that reason: the call form gives a kernel a private segment for the call's frame."""
from rustlight_amd import resources


def test_every_k_uplane_keeps_its_budget(built):
    rows = {(r["object"], r["kernel"]): r for r in resources.kernel_resources()}
    seen = 0
    for obj, lds in (("uplane_lds.hip.o", "true"), ("uplane_stream.hip.o", "false")):
        for mode in (0, 1, 2):                                 # a constant weight, DiscreteMIS, ContinousMIS
            r = rows[(obj, f"k_uplane<{lds}, {mode}>")]
            assert r["vgpr_spill"] == 0, r
            assert r["scratch_bytes_per_lane"] == 0, r
            assert r["max_waves_per_simd_by_vgpr"] >= 3, r
            seen += 1
    assert seen == 6 == sum(1 for (_, k) in rows if k.startswith("k_uplane<"))
