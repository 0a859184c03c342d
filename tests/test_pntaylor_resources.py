"""Register budgets of the point-normal Taylor kernels (kernels/pntaylor.hip.h), read from the code-object notes as tests/test_pn_resources.py does: the two
objects hold exactly pn.hip.h's drivers k_pn_pixel and k_pn_chain over the body PnTaylor<0..5> — every strategy's draw count depends on the data, so every one
has its chain kernel — each without VGPR spill and without a private segment; no kernel of another object carries that body, and none of these is a plain
(PnPlain<) or a MIS (PnMis<) kernel.  The waves per SIMD are recorded (profiles/r06_kernel_resources.csv, profiles/pntaylor_note.md), not set here: what is
held is that no strategy falls below three."""
from rustlight_amd import resources

KERNELS = [f"{k}<{{lds}}, PnTaylor<{s}> >" for k in ("k_pn_pixel", "k_pn_chain") for s in range(6)]


def test_point_normal_taylor_kernels_keep_their_budgets(built):
    rows = {(r["object"], r["kernel"]): r for r in resources.kernel_resources()}
    for obj, lds in (("pntaylor_lds.hip.o", "true"), ("pntaylor_stream.hip.o", "false")):
        want = {k.format(lds=lds) for k in KERNELS}
        assert {k for (o, k) in rows if o == obj} == want, obj
        for k in want:
            r = rows[(obj, k)]
            assert r["vgpr_spill"] == 0, r
            assert r["scratch_bytes_per_lane"] == 0, r
            assert r["max_waves_per_simd_by_vgpr"] >= 3, r
    assert sum(1 for (_, k) in rows if "PnTaylor<" in k) == 24
    assert not any("PnPlain<" in k or "PnMis<" in k for (o, k) in rows if o.startswith("pntaylor_"))
    assert not any("PnTaylor<" in k for (o, k) in rows if not o.startswith("pntaylor_"))
