"""Register budgets of the beam radiance estimate's gather (kernels/bre.hip.h), read from the code-object notes like tests/test_vpl_resources.py does."""
from rustlight_amd import resources


def test_bre_gather_keeps_its_budget(built):
    rows = {(r["object"], r["kernel"]): r for r in resources.kernel_resources()}
    for obj, lds in (("bre_lds.hip.o", "true"), ("bre_stream.hip.o", "false")):
        for hg in ("false", "true"):
            r = rows[(obj, f"k_bre_gather<{lds}, {hg}>")]
            assert r["vgpr_spill"] == 0, r
            assert r["vgpr"] <= 128, r                      # four waves per SIMD, the budget k_vpl_gather is held to
            assert r["scratch_bytes_per_lane"] == 0, r      # no private segment
