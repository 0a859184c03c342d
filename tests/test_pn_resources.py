"""Register budgets of the point-normal kernels (kernels/pn.hip.h), read from the code-object notes like tests/test_uplane_resources.py does: every
instantiation of k_pn_pixel over PnPlain<STRATEGY> without VGPR spill, without a private segment and within 128 VGPRs; every k_pn_chain without spill and
without a private segment; and the two objects hold exactly these kernels.  rng_advance<false> keeps the jump table's step in line, the use_aa flag is read
at run time, and a lane parks its sampler and its pixel sum in memory between samples for these budgets.  (The drivers are templates over the sample body and
pnmis.hip.h instantiates them too: the body's name, PnPlain< or PnMis<, is what tells a kernel's kind.)"""
from rustlight_amd import resources

PIXEL = [f"k_pn_pixel<{{lds}}, PnPlain<{s}> >" for s in range(7)]                  # rl_pn_strategy 0 .. 6
CHAIN = [f"k_pn_chain<{{lds}}, PnPlain<{s}> >" for s in (4, 5, 6)]                 # eq_clamped_ex, eq_clamped_phase, pn_ex: the data-dependent draw counts


def test_point_normal_kernels_keep_their_budgets(built):
    rows = {(r["object"], r["kernel"]): r for r in resources.kernel_resources()}
    for obj, lds in (("pn_lds.hip.o", "true"), ("pn_stream.hip.o", "false")):
        want = {k.format(lds=lds) for k in PIXEL + CHAIN}
        assert {k for (o, k) in rows if o == obj} == want, obj
        for k in want:
            r = rows[(obj, k)]
            assert r["vgpr_spill"] == 0, r
            assert r["scratch_bytes_per_lane"] == 0, r
            if k.startswith("k_pn_pixel"):
                assert r["vgpr"] + r["agpr"] <= 128 and r["max_waves_per_simd_by_vgpr"] >= 4, r
    assert sum(1 for (_, k) in rows if "PnPlain<" in k) == 20
