"""Register budgets of the photon beams' kernels, read from the code-object notes like tests/test_bre_resources.py does: the gather (kernels/beam.hip.h) keeps
the budget k_bre_gather is held to; the generation kernels (kernels/beamgen.hip.h) have no private segment — their register numbers stand in
profiles/beam_note.md beside k_vpl_generate's."""
from rustlight_amd import resources


def test_beam_gather_keeps_its_budget(built):
    rows = {(r["object"], r["kernel"]): r for r in resources.kernel_resources()}
    for obj, lds in (("beam_lds.hip.o", "true"), ("beam_stream.hip.o", "false")):
        r = rows[(obj, f"k_beam_gather<{lds}>")]
        assert r["vgpr_spill"] == 0, r
        assert r["vgpr"] <= 128, r                      # four waves per SIMD
        assert r["scratch_bytes_per_lane"] == 0, r      # no private segment


def test_beam_generation_has_no_private_segment(built):
    rows = [r for r in resources.kernel_resources() if r["object"] in ("beamgen_lds.hip.o", "beamgen_stream.hip.o")]
    names = {r["kernel"].split("<")[0] for r in rows}
    assert names == {"k_beam_generate", "k_beam_shoot"} and len(rows) == 2 * (6 + 12)      # six BSDF dispatches; the shoot kernel in a count and a write form
    for r in rows:
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0, r
