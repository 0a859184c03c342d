"""Register budgets of the virtual ray lights' kernels, read from the code-object notes like tests/test_beam_resources.py does.  The gather (kernels/vrl.hip.h)
is held to k_beam_gather's budget — no VGPR spill, no private segment, at most 128 VGPRs — with the four-entry queue in registers; the chain pass has no spill
and no private segment.  The two new objects hold the new kernels and nothing else: every existing object keeps the kernel set the other resources tests pin."""
from rustlight_amd import resources


def test_vrl_gather_keeps_its_budget(built):
    rows = {(r["object"], r["kernel"]): r for r in resources.kernel_resources()}
    for obj, lds in (("vrl_lds.hip.o", "true"), ("vrl_stream.hip.o", "false")):
        r = rows[(obj, f"k_vrl_gather<{lds}>")]
        assert r["vgpr_spill"] == 0, r
        assert r["scratch_bytes_per_lane"] == 0, r      # no private segment
        assert r["vgpr"] <= 128, r
    assert sum(1 for (_, k) in rows if k.startswith("k_vrl_gather<")) == 2


def test_vrl_chain_has_no_private_segment(built):
    rows = [r for r in resources.kernel_resources() if r["kernel"].startswith("k_vrl_chain")]
    assert len(rows) == 1 and rows[0]["object"] == "vrl_lds.hip.o", rows
    assert rows[0]["vgpr_spill"] == 0 and rows[0]["scratch_bytes_per_lane"] == 0, rows[0]


def test_the_new_objects_hold_the_new_kernels_only(built):
    names = sorted(r["kernel"] for r in resources.kernel_resources() if r["object"] in ("vrl_lds.hip.o", "vrl_stream.hip.o"))
    assert names == ["k_vrl_chain", "k_vrl_gather<false>", "k_vrl_gather<true>"], names
