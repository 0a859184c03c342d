"""The workload of profiles/uplane_note.md: cbox_medium 1920 x 1080 (sigma_s = 0.5), 1 spp, seed 0, 128 planes per camera sample, average and cmis through
rl_render_plane_uncorrelated.  Prints one JSON line per strategy: ms_other of every render (the first is the warm-up), the counters of the last.
`--renders N` sets how many (default 6); under a profiler run it with `--renders 2` as the program after `--`."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rustlight_amd import api, scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--renders", type=int, default=6)
ap.add_argument("--planes", type=int, default=128)
args = ap.parse_args()
sd = scenes.cbox_medium(1920, 1080, 0.5)
ctx = api.Context(api.Scene(sd), 0)
seeds = api.IndependentSampler(0).block_seeds(1920, 1080)
for strategy in ("average", "cmis"):
    ms, st = [], None
    for _ in range(args.renders):
        _, st = ctx.render_plane_uncorrelated(seeds, args.planes, strategy, 1)
        ms.append(round(st["ms_other"], 3))
    keep = ("camera_samples", "rng_draws", "redraws", "planes_intersected", "planes_visible", "shadow_rays")
    print(json.dumps({"strategy": strategy, "planes": args.planes, "ms_other": ms, **{k: st[k] for k in keep}}), flush=True)
