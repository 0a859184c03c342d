"""A small seeded fuzz of rl_render_point_normal_mis against tests/pnmis_restatement.py, in the size of tests/test_gpu_pn_fuzz.py: 24 cases with a random
strategy name, AA, stream mode, scene (the box, the box with a second area light and a point light, the floating light), medium colour, absorption and phase
function, frame up to 40 x 40, up to 4 spp, 1 to 3 shards; one case in sixteen on average carries something both sides refuse (a directional light, the light
tree, no medium) and must be refused with the same code.  Image and counters bit for bit.  The CPU test holds the chosen seed to at most a tenth of refused
cases and to every family, stream mode, shard count and scene being drawn."""
import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import pn_restatement as P
from tests import pnmis_restatement as M
from tests.scene_helpers import context as _context

SEED, N_CASES = 20263, 24


def cases():
    rng = np.random.default_rng(SEED)
    out = []
    for i in range(N_CASES):
        c = {"i": i, "strategy": P.STRATEGIES[rng.integers(7)], "use_aa": bool(rng.integers(2)), "mode": int(rng.integers(2)),
             "scene": ("box", "lights", "floating")[rng.integers(3)], "w": int(rng.integers(1, 41)), "h": int(rng.integers(1, 41)), "spp": int(rng.integers(1, 5)),
             "shards": int(rng.integers(1, 4)), "seed": int(rng.integers(1 << 30))}
        grey = bool(rng.integers(2))
        ss = rng.uniform(0.2, 2.0, 1 if grey else 3)
        sa = rng.uniform(0.0, 1.0, 1 if grey else 3) * rng.integers(2)
        c["sigma_s"], c["sigma_a"] = tuple(np.resize(ss, 3).tolist()), tuple(np.resize(sa, 3).tolist())
        c["g"] = None if rng.integers(2) else float(rng.uniform(-0.8, 0.8))
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


def test_the_seed_keeps_refusals_rare_and_draws_every_family():
    cs = cases()
    assert len(cs) == N_CASES and sum(c["refuse"] is not None for c in cs) <= N_CASES // 10
    assert {M.family(c["strategy"]) for c in cs} == set(M.FAMILIES) and {c["mode"] for c in cs} == {0, 1} and {c["use_aa"] for c in cs} == {True, False}
    assert {c["shards"] for c in cs} == {1, 2, 3} and {c["scene"] for c in cs} == {"box", "lights", "floating"}
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
    if c["refuse"]:
        with pytest.raises(P.Refused) as want:
            M.Frame(sd)
        with pytest.raises(api.RustlightError) as got:
            ctx.render_point_normal_mis(seeds, c["strategy"], c["spp"], c["use_aa"], c["mode"])
        assert got.value.code == want.value.code
        return
    fr = M.Frame(sd)
    for shard in range(c["shards"]):
        ref, st, det = M.render(fr, seeds, c["strategy"], c["spp"], c["use_aa"], c["mode"], 0, shard, c["shards"])
        img, got = ctx.render_point_normal_mis(seeds, c["strategy"], c["spp"], c["use_aa"], c["mode"], 0, shard, c["shards"])
        assert img.tobytes() == ref.tobytes(), (c, shard, int((img != ref).any(axis=2).sum()))
        assert {k: got[k] for k in M.COUNTERS} == st, (c, shard)
