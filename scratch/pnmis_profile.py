"""The workload of profiles/pnmis_note.md: cbox_medium 1920 x 1080 (sigma_s = 0.5), 4 spp, seed 0, one name of each point-normal-mis family in both stream
modes through rl_render_point_normal_mis.  Prints one JSON line per (family, stream mode): ms_other (k_pnmis_pixel) and ms_prepass (k_pnmis_chain) of every
render (the first is the warm-up), the counters of the last.  `--renders N` sets how many (default 4); under a profiler run it with `--renders 2` as the
program after `--`."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rustlight_amd import api, scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--renders", type=int, default=4)
ap.add_argument("--spp", type=int, default=4)
args = ap.parse_args()
sd = scenes.cbox_medium(1920, 1080, 0.5)
ctx = api.Context(api.Scene(sd), 0)
seeds = api.IndependentSampler(0).block_seeds(1920, 1080)
for family, strategy in (("tr", "tr_ex"), ("eq", "eq_ex"), ("clamped", "eq_clamped_ex"), ("pn", "pn_ex")):
    for mode, name in ((api.STREAM_REFERENCE_ORDER, "reference"), (api.STREAM_PER_SAMPLE, "per-sample")):
        ms, pre, st = [], [], None
        for _ in range(args.renders):
            _, st = ctx.render_point_normal_mis(seeds, strategy, args.spp, True, mode)
            ms.append(round(st["ms_other"], 3)); pre.append(round(st["ms_prepass"], 3))
        keep = ("camera_samples", "rng_draws", "extension_rays", "shadow_rays", "vertices", "kernel_launches")
        print(json.dumps({"family": family, "streams": name, "spp": args.spp, "ms_pixel": ms, "ms_chain": pre, **{k: st[k] for k in keep}}), flush=True)
