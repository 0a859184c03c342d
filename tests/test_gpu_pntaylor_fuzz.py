"""A small seeded fuzz of rl_render_point_normal_taylor against tests/pntaylor_restatement.py, in the size of tests/test_gpu_pn_fuzz.py: 24 cases with a random
strategy, AA, stream mode, scene (the box, the box with a second area light and a point light, the floating light), medium colour, absorption and phase
function — isotropic, Henyey-Greenstein with a random g, or Henyey-Greenstein with g = 0 —, frame up to 40 x 40, up to 4 spp, 1 to 3 shards; one case in
sixteen on average carries something both sides refuse (a directional light, the light tree, no medium), and pn_phase_taylor_ex with g = 0 is refused by both
with the same code.  Image and counters bit for bit.  The CPU test holds the chosen seed to every strategy, stream mode, shard count, scene and kind of medium
being drawn and to refusals staying rare."""
import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import pn_restatement as P
from tests import pntaylor_restatement as T
from tests.scene_helpers import context as _context

SEED, N_CASES = 20270, 24


def cases():
    rng = np.random.default_rng(SEED)
    out = []
    for i in range(N_CASES):
        c = {"i": i, "strategy": T.STRATEGIES[rng.integers(6)], "use_aa": bool(rng.integers(2)), "mode": int(rng.integers(2)),
             "scene": ("box", "lights", "floating")[rng.integers(3)], "w": int(rng.integers(1, 41)), "h": int(rng.integers(1, 41)), "spp": int(rng.integers(1, 5)),
             "shards": int(rng.integers(1, 4)), "seed": int(rng.integers(1 << 30))}
        grey = bool(rng.integers(2))
        ss = rng.uniform(0.2, 2.0, 1 if grey else 3)
        sa = rng.uniform(0.0, 1.0, 1 if grey else 3) * rng.integers(2)
        c["sigma_s"], c["sigma_a"] = tuple(np.resize(ss, 3).tolist()), tuple(np.resize(sa, 3).tolist())
        kind = int(rng.integers(4))                                                          # 0 isotropic | 1 Henyey-Greenstein with g = 0 | 2, 3 a random g
        c["g"] = None if kind == 0 else (0.0 if kind == 1 else float(rng.uniform(-0.8, 0.8)))
        c["refuse"] = (None, "directional", "ats", "no medium")[rng.integers(1, 4)] if rng.random() < 1.0 / 16.0 else None
        out.append(c)
    return out


def build(c):
    sd = P.scene(c["scene"], c["w"], c["h"])
    sd.medium = scenes.Medium(c["sigma_a"], c["sigma_s"], scenes.PHASE_ISOTROPIC if c["g"] is None else scenes.PHASE_HG, 0.0 if c["g"] is None else c["g"])
    if c["refuse"] == "directional":
        sd.lights.append({"type": "directional", "a": (0.0, -1.0, 0.0), "intensity": (1.0, 1.0, 1.0)})
    elif c["refuse"] == "ats":
        sd.use_ats = True
    elif c["refuse"] == "no medium":
        sd.medium = None
    return sd


def g_is_zero(c):
    return c["strategy"] == "pn_phase_taylor_ex" and not c["g"]


def test_the_seed_draws_every_strategy_and_keeps_refusals_rare():
    cs = cases()
    assert len(cs) == N_CASES and sum(c["refuse"] is not None for c in cs) <= N_CASES // 10
    assert sum(g_is_zero(c) for c in cs) <= N_CASES // 10 and sum(c["refuse"] is not None or g_is_zero(c) for c in cs) <= N_CASES // 6
    assert {c["strategy"] for c in cs} == set(T.STRATEGIES) and {c["mode"] for c in cs} == {0, 1} and {c["use_aa"] for c in cs} == {True, False}
    assert {c["shards"] for c in cs} == {1, 2, 3} and {c["scene"] for c in cs} == {"box", "lights", "floating"}
    assert {"none" if c["g"] is None else ("zero" if c["g"] == 0.0 else "g") for c in cs} == {"none", "zero", "g"}
    # a phase polynomial is drawn in a medium with g != 0, the forwarding and the g = 0 refusal are drawn too
    assert any(T.is_phase_poly(c["strategy"]) and c["g"] and not c["refuse"] for c in cs)
    assert any(c["strategy"] in ("eq_phase_taylor_ex", "eq_clamped_phase_taylor_ex") and c["g"] is None and not c["refuse"] for c in cs)
    for c in cs:
        if c["refuse"]:
            with pytest.raises(P.Refused):
                P.check_scene(build(c))
        else:
            P.check_scene(build(c))


@pytest.mark.gpu
@pytest.mark.parametrize("c", cases(), ids=lambda c: f"{c['i']}-{c['strategy']}-{c['scene']}")
def test_fuzz_case(built, c):
    sd = build(c)
    seeds = orc.block_seeds(c["seed"], c["w"], c["h"])
    ctx = _context(sd)
    if c["refuse"] or g_is_zero(c):
        with pytest.raises(P.Refused) as want:
            T.render(T.Frame(sd), seeds, c["strategy"], c["spp"], c["use_aa"], c["mode"])
        with pytest.raises(api.RustlightError) as got:
            ctx.render_point_normal_taylor(seeds, c["strategy"], c["spp"], c["use_aa"], c["mode"])
        assert got.value.code == want.value.code
        return
    fr = T.Frame(sd)
    for shard in range(c["shards"]):
        ref, st, det = T.render(fr, seeds, c["strategy"], c["spp"], c["use_aa"], c["mode"], 0, shard, c["shards"])
        img, got = ctx.render_point_normal_taylor(seeds, c["strategy"], c["spp"], c["use_aa"], c["mode"], 0, shard, c["shards"])
        assert img.tobytes() == ref.tobytes(), (c, shard, int((img != ref).any(axis=2).sum()))
        assert {k: got[k] for k in T.COUNTERS} == st, (c, shard)
