"""Register budgets of the point-normal kernels over the light tree (kernels/pnats.hip.h), read from the code-object notes as tests/test_pntaylor_resources.py
does: the two objects hold exactly pn.hip.h's drivers over the body PnAts<family, strategy> — k_pn_pixel for the seven plain and the six Taylor names,
k_pn_chain for the three plain strategies whose sampler can be None and for every Taylor name — each without VGPR spill and without a private segment at
the wave count it is committed at (pnats_waves: four, three for the Taylor names but pn_tr_taylor_ex; profiles/pnats_note.md says why); no kernel of another
object carries that body, and none of these is a plain (PnPlain<), a MIS (PnMis<) or a Taylor (PnTaylor<) kernel."""
from rustlight_amd import resources

PLAIN, TAYLOR = [(0, s) for s in range(7)], [(1, s) for s in range(6)]
PIXEL = [f"k_pn_pixel<{{lds}}, PnAts<{f}, {s}> >" for f, s in PLAIN + TAYLOR]
CHAIN = [f"k_pn_chain<{{lds}}, PnAts<{f}, {s}> >" for f, s in [(0, 4), (0, 5), (0, 6)] + TAYLOR]
THREE_WAVES = {f"PnAts<1, {s}>" for s in (0, 1, 2, 3, 5)}


def test_point_normal_ats_kernels_keep_their_budgets(built):
    rows = {(r["object"], r["kernel"]): r for r in resources.kernel_resources()}
    for obj, lds in (("pnats_lds.hip.o", "true"), ("pnats_stream.hip.o", "false")):
        want = {k.format(lds=lds) for k in PIXEL + CHAIN}
        assert {k for (o, k) in rows if o == obj} == want, obj
        for k in want:
            r = rows[(obj, k)]
            assert r["vgpr_spill"] == 0, r
            assert r["scratch_bytes_per_lane"] == 0, r
            committed = 3 if k.startswith("k_pn_pixel") and any(b in k for b in THREE_WAVES) else 4
            assert r["max_waves_per_simd_by_vgpr"] >= committed, r
    assert sum(1 for (_, k) in rows if "PnAts<" in k) == 44
    assert not any("PnPlain<" in k or "PnMis<" in k or "PnTaylor<" in k for (o, k) in rows if o.startswith("pnats_"))
    assert not any("PnAts<" in k for (o, k) in rows if not o.startswith("pnats_"))
