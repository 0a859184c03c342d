"""Writes tests/golden/gather_high_counter.json: what the restatement of the beam radiance estimate (tests/bre_restatement.py) gives for the one lane of a
1x1 frame whose two walk counters pass 2^24 — cbox_medium(1, 1, 1.0), seed 3, 2048 photons of radius 2.0 — at the smallest multiple of 1024 spp for which
nodes_entered and photons_gathered both reach 2^24: the pixel (its bits) and the five counters, and the two counters one step of 1024 spp below, which shows
that the step is the smallest.  tests/test_gpu_gather_edges.py holds rl_render_bre to it; the restatement takes about 0.8 s per 1024 spp, too long for a test.
usage: python tests/golden/make_gather_high_counter.py      (about a minute, no GPU)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from rustlight_amd import scenes            # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gather_high_counter.json")
CASE = dict(seed=3, nb_primitive=2048, radius=2.0)
KEYS = ("camera_samples", "extension_rays", "rng_draws", "nodes_entered", "photons_gathered")
STEP, BAR = 1024, 1 << 24


def scene():
    return scenes.cbox_medium(1, 1, 1.0)


if __name__ == "__main__":
    from tests import bre_restatement as R

    def at(spp):
        r = R.compute(scene(), spp=spp, **CASE)
        print(spp, {k: r["stats"][k] for k in KEYS}, flush=True)
        return r

    first = at(STEP)["stats"]
    k = -(-BAR * STEP // min(first["nodes_entered"], first["photons_gathered"])) // STEP       # from the rates of the first 1024 samples
    reached = lambda st: st["nodes_entered"] >= BAR and st["photons_gathered"] >= BAR
    r = at(k * STEP)
    while not reached(r["stats"]):
        k += 1
        r = at(k * STEP)
    below = at((k - 1) * STEP)["stats"]
    while reached(below):
        k -= 1
        r, below = at(k * STEP), at((k - 1) * STEP)["stats"]
    out = {"case": dict(CASE, width=1, height=1, sigma_s=1.0), "spp": k * STEP, "pixel_bits": [int(v) for v in r["image"].reshape(3).view(np.uint32)],
           "stats": {key: int(r["stats"][key]) for key in KEYS}, "records": int(r["records"].shape[0]), "n_paths": int(r["n_paths"]),
           "below": {"spp": (k - 1) * STEP, "nodes_entered": int(below["nodes_entered"]), "photons_gathered": int(below["photons_gathered"])}}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(out)
