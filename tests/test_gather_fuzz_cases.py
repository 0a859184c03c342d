"""What the light-pass arms of tests/parity_fuzz.py ("vpl", "bre", "plane") and the camera-beam gather lean on, checked without a GPU: the case generators
reach what they claim to reach (every strategy, both phase functions, both tree builds, both stream kinds, a zero absorption channel, single-column and
single-row frames, shards of 2, 3 and 4) and their scenes render (the restatements alone refuse at most a tenth of the cases and leave few images black);
and the statistics rows the gather's leaves name in kernels/launch.h are pairwise distinct within a leaf and inside the block's row count."""
import os
import re

import numpy as np
import pytest

from rustlight_amd import api
from tests import parity_fuzz as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "rustlight_amd", "csrc", "kernels")
N_CASES = 300


def _cases(arm, n=N_CASES):
    rng = np.random.default_rng(2024)
    return [F.draw_gather_case(rng, arm) for _ in range(n)]


@pytest.mark.parametrize("arm", F.GATHER_ARMS)
def test_generators_reach_what_they_claim(arm):
    cases = _cases(arm)
    sizes = [c["size"] for c in cases]
    assert all(1 <= w <= 48 and 1 <= h <= 40 for w, h in sizes)
    assert any(w == 1 for w, _ in sizes) and any(h == 1 for _, h in sizes)
    assert 5 * sum(w in F.EDGE_SIZES or h in F.EDGE_SIZES for w, h in sizes) >= len(cases)
    assert {c["shard_count"] for c in cases} == {1, 2, 3, 4} and all(c["shard_index"] < c["shard_count"] and F.owned_samples(c) > 0 for c in cases)
    assert any(c["shard_index"] == 3 for c in cases)
    assert 0.15 * len(cases) <= sum(c["shard_count"] > 1 for c in cases) <= 0.35 * len(cases)
    assert {c["seed_variant"] for c in cases} == {0, 1} and {c["spp"] for c in cases} == {1, 2, 3, 4, 5}
    assert {c["streaming"] for c in cases} == {False, True}
    media = [c["medium"] for c in cases if c["medium"] is not None]
    assert len(media) == len(cases) if arm != "vpl" else 0.2 * len(cases) <= len(media) <= 0.5 * len(cases)
    assert {m["hg"] for m in media} == {False, True}
    assert any(m["g"] < -0.3 for m in media) and any(m["g"] > 0.3 for m in media) and all(-0.7 <= m["g"] <= 0.7 for m in media)
    assert any(0.0 in m["sigma_a"] for m in media)
    assert all(0.0 <= a <= 0.3 for m in media for a in m["sigma_a"]) and all(0.1 <= s <= 1.5 for m in media for s in m["sigma_s"])
    assert all(len(set(m["sigma_s"])) == 3 for m in media)
    if arm == "plane":
        assert {c["strategy"] for c in cases} == set(api.PLANE_STRATEGIES) and len(api.PLANE_STRATEGIES) == 7
        assert {c["two_lights"] for c in cases} == {False, True}
        assert min(c["nb_primitive"] for c in cases) >= 3 and max(c["nb_primitive"] for c in cases) <= 200
        return
    assert {c["per_path"] for c in cases} == {False, True}
    assert {c["vpl_batch_paths"] for c in cases if c["per_path"]} == set(F.VPL_BATCHES)
    assert any(c["max_depth"] is None for c in cases) and any(c["rr_depth"] is None for c in cases)
    assert all(c["max_depth"] is not None or c["rr_depth"] is not None for c in cases)
    if arm == "vpl":
        assert {(c["option_vpl"], c["option_lt"]) for c in cases} == {(a, b) for a in range(3) for b in range(3)}
        assert min(c["nb_vpl"] for c in cases) >= 1 and max(c["nb_vpl"] for c in cases) <= 128
    else:
        assert {c["device_build"] for c in cases} == {False, True}
        assert {c["photon_tree_group_photons"] for c in cases if c["device_build"]} == set(F.TREE_GROUPS)
        assert all(g is None or 4 <= g <= api.PHOTON_TREE_GROUP_PHOTONS for g in F.TREE_GROUPS)
        assert min(c["nb_primitive"] for c in cases) >= 1 and max(c["nb_primitive"] for c in cases) <= 400
        assert all(0.02 <= c["radius"] <= 0.5 for c in cases)


def test_a_case_is_a_function_of_its_values():
    """What a MISMATCH line prints replays: the scene comes from the case alone."""
    for arm in F.GATHER_ARMS:
        c = _cases(arm, 3)[2]
        a, b = F.gather_scene(c), F.gather_scene(eval(repr(c)))
        assert (a.width, a.height) == c["size"] and len(a.meshes) == len(b.meshes)
        assert [repr(m.bsdf) for m in a.meshes] == [repr(m.bsdf) for m in b.meshes]
        assert repr(a.medium) == repr(b.medium)


def test_vpl_scenes_are_ones_the_generation_accepts(built):
    kinds = set()
    for c in _cases("vpl", 60):
        sd = F.gather_scene(c)
        assert sd.environment is None and getattr(sd, "environment_map", None) is None
        assert any(m.emission is not None for m in sd.meshes) or sd.lights
        assert sd.medium is not None or c["option_vpl"] != api.VPL_VOLUME
        assert sd.medium is None or not any(l.get("type") == "directional" for l in sd.lights)
        kinds.add((len(sd.meshes), bool(sd.lights), sd.medium is not None))
    assert len(kinds) >= 6                                      # several scene kinds, with and without lights and media


@pytest.mark.parametrize("arm", ["bre", "plane"])
def test_the_restatements_render_the_first_cases(built, arm):
    refs = [F.gather_reference(c) for c in _cases(arm, 40)]
    rendered = [r for r in refs if not r.get("refused")]
    assert 10 * sum(bool(r.get("refused")) for r in refs) <= len(refs)
    assert all(np.isfinite(r["image"]).all() for r in rendered)
    assert 10 * sum(bool(r["image"].any()) for r in rendered) >= 9 * len(rendered), [bool(r["image"].any()) for r in rendered]


# ---- the statistics rows of the gather (kernels/launch.h, kernels/pathstate.hip.h)
def _enumerators(text):
    """{name: value} of every `enum { A, B = 3, C }` in the text."""
    out = {}
    for body in re.findall(r"enum\s*\{([^}]*)\}", text):
        nxt = 0
        for item in body.split(","):
            m = re.match(r"\s*(\w+)\s*(?:=\s*(\w+))?\s*$", item)
            if not m:
                continue
            nxt = int(m.group(2), 0) if m.group(2) and m.group(2)[0].isdigit() else (out[m.group(2)] if m.group(2) else nxt)
            out[m.group(1)] = nxt
            nxt += 1
    return out


def test_gather_statistics_rows():
    launch = open(os.path.join(KERNELS, "launch.h")).read()
    stats = _enumerators(open(os.path.join(KERNELS, "pathstate.hip.h")).read())
    rows = _enumerators(launch)
    n_rows = stats["STAT_COUNT"]
    assert n_rows == 8 and stats["STAT_SAMPLES"] == 0
    leaves = {}
    for header, leaf in (("bre.hip.h", "BreLeaf"), ("plane.hip.h", "PlaneLeaf")):
        text = open(os.path.join(KERNELS, header)).read()
        m = re.search(r"kLo\[\d\]\s*=\s*\{([^}]*)\}\s*,\s*kHi\[\d\]\s*=\s*\{([^}]*)\}", text[text.index("struct " + leaf):])
        lo, hi = ([name.strip() for name in group.split(",")] for group in m.groups())
        k = int(re.search(r"kCounters\s*=\s*(\d+)", text).group(1))
        assert len(lo) == len(hi) == k
        leaves[leaf] = lo + hi
    assert len(leaves["BreLeaf"]) == 2 and len(leaves["PlaneLeaf"]) == 4
    for leaf, names in leaves.items():
        used = ["STAT_SAMPLES", "STAT_GATHER_NODES", "STAT_GATHER_NODES_HI"] + names
        values = [dict(stats, **rows)[name] for name in used]
        assert len(set(values)) == len(values), (leaf, dict(zip(used, values)))
        assert all(0 <= v < n_rows for v in values), (leaf, dict(zip(used, values)))
    # the host joins the rows the kernels split (gather_render.hip.h: GatherKind) by the same names
    host = open(os.path.join(KERNELS, "gather_render.hip.h")).read()
    assert "{STAT_BRE_PHOTONS}, {STAT_BRE_PHOTONS_HI}" in host
    assert "{STAT_PLANE_ISECT, STAT_PLANE_VISIBLE}, {STAT_PLANE_ISECT_HI, STAT_PLANE_VISIBLE_HI}" in host
    assert "gather_merge24(fr.totals, STAT_GATHER_NODES, STAT_GATHER_NODES_HI)" in host
