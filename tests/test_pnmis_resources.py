"""Register budgets of the point-normal MIS kernels (kernels/pnmis.hip.h), read from the code-object notes as tests/test_pn_resources.py does: the two
objects hold exactly pn.hip.h's drivers over the body PnMis<FAMILY> — k_pn_pixel for the four families (0 tr, 1 eq, 2 clamped, 3 pn), k_pn_chain for the two
data-dependent ones — each without VGPR spill and without a private segment; no kernel of another object carries that body, and none of these is a plain
(PnPlain<) kernel.  The waves per SIMD are recorded (profiles/r06_kernel_resources.csv, profiles/pnmis_note.md), not set here: what is held is that no family
falls below three."""
from rustlight_amd import resources

PIXEL = [f"k_pn_pixel<{{lds}}, PnMis<{f}> >" for f in range(4)]
CHAIN = [f"k_pn_chain<{{lds}}, PnMis<{f}> >" for f in (2, 3)]


def test_point_normal_mis_kernels_keep_their_budgets(built):
    rows = {(r["object"], r["kernel"]): r for r in resources.kernel_resources()}
    for obj, lds in (("pnmis_lds.hip.o", "true"), ("pnmis_stream.hip.o", "false")):
        want = {k.format(lds=lds) for k in PIXEL + CHAIN}
        assert {k for (o, k) in rows if o == obj} == want, obj
        for k in want:
            r = rows[(obj, k)]
            assert r["vgpr_spill"] == 0, r
            assert r["scratch_bytes_per_lane"] == 0, r
            assert r["max_waves_per_simd_by_vgpr"] >= 3, r
        # the transmittance family runs at point-normal's four waves
        r = rows[(obj, PIXEL[0].format(lds=lds))]
        assert r["vgpr"] + r["agpr"] <= 128 and r["max_waves_per_simd_by_vgpr"] >= 4, r
    assert sum(1 for (_, k) in rows if "PnMis<" in k) == 12
    assert not any("PnPlain<" in k for (o, k) in rows if o.startswith("pnmis_"))
