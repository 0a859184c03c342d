"""Register budgets of the light tracer's kernels (kernels/light.hip.h), read from the code-object notes like tests/test_resources.py does."""
from rustlight_amd import resources


def test_light_kernels_keep_their_budgets(built):
    rows = {(r["object"], r["kernel"]): r for r in resources.kernel_resources()}
    cbox = rows[("light_lds.hip.o", "k_light_fused<0, true, false>")]        # the diffuse Cornell box
    assert cbox["vgpr_spill"] == 0 and cbox["max_waves_per_simd_by_vgpr"] >= 4
    for obj in ("light_lds.hip.o", "light_stream.hip.o"):
        for mat in (-1, 0, 1, 2, 3, 4):
            for medium in ("false", "true"):
                r = rows[(obj, f"k_light_fused<{mat}, {'true' if obj == 'light_lds.hip.o' else 'false'}, {medium}>")]
                assert r["max_waves_per_simd_by_vgpr"] >= 4 and r["vgpr"] <= 128
    assert rows[("light_lds.hip.o", "k_light_resolve")]["vgpr_spill"] == 0
