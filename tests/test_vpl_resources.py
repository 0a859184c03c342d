"""Register budgets of the VPL kernels (kernels/vpl.hip.h), read from the code-object notes like tests/test_resources.py does."""
from rustlight_amd import resources


def test_vpl_kernels_keep_their_budgets(built):
    rows = {(r["object"], r["kernel"]): r for r in resources.kernel_resources()}
    for k in ("k_vpl_generate<0, true, false>", "k_vpl_gather<0, true, false>", "k_vpl_primary<true, false>"):     # the diffuse Cornell box
        r = rows[("vpl_lds.hip.o", k)]
        assert r["vgpr_spill"] == 0 and r["vgpr"] <= 128, (k, r)
    assert rows[("vpl_lds.hip.o", "k_vpl_gather<0, true, false>")]["max_waves_per_simd_by_vgpr"] >= 5
    for obj, lds in (("vpl_lds.hip.o", "true"), ("vpl_stream.hip.o", "false")):
        for mat in (-1, 0, 1, 2, 3, 4):
            for medium in ("false", "true"):
                r = rows[(obj, f"k_vpl_gather<{mat}, {lds}, {medium}>")]
                assert r["max_waves_per_simd_by_vgpr"] >= 4 and r["vgpr"] <= 128, r
                assert rows[(obj, f"k_vpl_generate<{mat}, {lds}, {medium}>")]["vgpr"] <= 256
    assert rows[("vpl_lds.hip.o", "k_vpl_resolve")]["vgpr_spill"] == 0
