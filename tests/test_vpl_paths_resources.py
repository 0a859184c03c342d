"""Register budgets of the per-path light-path kernel (kernels/vpl_paths.hip.h), read from the code-object notes like tests/test_vpl_resources.py does: every
instantiation of k_vpl_shoot without spill and without a private segment, at three waves per SIMD or more — what the serial kernel, the same walk, meets."""
from rustlight_amd import resources


def test_every_k_vpl_shoot_keeps_its_budget(built):
    rows = {(r["object"], r["kernel"]): r for r in resources.kernel_resources()}
    seen = 0
    for obj, lds in (("vpl_paths_lds.hip.o", "true"), ("vpl_paths_stream.hip.o", "false")):
        for mat in (-1, 0, 1, 2, 3, 4):
            for medium in ("false", "true"):
                for write in ("false", "true"):
                    r = rows[(obj, f"k_vpl_shoot<{mat}, {lds}, {medium}, {write}>")]
                    assert r["vgpr_spill"] == 0, r
                    assert r["scratch_bytes_per_lane"] == 0, r
                    assert r["max_waves_per_simd_by_vgpr"] >= 3, r
                    seen += 1
    assert seen == 48 == sum(1 for (_, k) in rows if k.startswith("k_vpl_shoot<"))
