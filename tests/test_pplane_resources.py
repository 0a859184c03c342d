"""Register budgets of the photon planes' kernels, read from the code-object notes like tests/test_plane_single_resources.py does.  The gather
(kernels/pplane.hip.h) holds a scene traversal in its plane leaf, so its bar is k_plane_gather's: no VGPR spill, no private segment, three waves per SIMD or
more.  The generation kernels (kernels/pplanegen.hip.h) have no private segment.  The four new objects hold the new kernels and nothing else: every existing
object keeps the kernel set the other resources tests pin."""
from rustlight_amd import resources


def test_pplane_gather_keeps_its_budget(built):
    rows = {(r["object"], r["kernel"]): r for r in resources.kernel_resources()}
    for obj, lds in (("pplane_lds.hip.o", "true"), ("pplane_stream.hip.o", "false")):
        r = rows[(obj, f"k_pplane_gather<{lds}>")]
        assert r["vgpr_spill"] == 0, r
        assert r["scratch_bytes_per_lane"] == 0, r      # no private segment
        assert r["max_waves_per_simd_by_vgpr"] >= 3, r
    in_objects = [k for (o, k) in rows if o in ("pplane_lds.hip.o", "pplane_stream.hip.o")]
    assert len(in_objects) == 2 and all(k.startswith("k_pplane_gather<") for k in in_objects), in_objects
    assert sum(1 for (_, k) in rows if k.startswith("k_pplane_gather<")) == 2


def test_pplane_generation_has_no_private_segment(built):
    rows = [r for r in resources.kernel_resources() if r["object"] in ("pplanegen_lds.hip.o", "pplanegen_stream.hip.o")]
    names = {r["kernel"].split("<")[0] for r in rows}
    assert names == {"k_pplane_generate", "k_pplane_shoot"} and len(rows) == 2 * (6 + 12)      # six BSDF dispatches; the shoot kernel in a count and a write form
    for r in rows:
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0, r
