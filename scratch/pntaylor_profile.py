"""The workload of profiles/pntaylor_note.md: cbox_medium 1920 x 1080 (sigma_s = 0.5), 4 spp, seed 0, the six point-normal-taylor strategies in both stream
modes through rl_render_point_normal_taylor and, in the same process, the plain eq_ex, eq_clamped_ex and pn_ex through rl_render_point_normal.  `--g G` makes
the medium Henyey-Greenstein with that g (the phase polynomials: in the isotropic medium the two eq ones are the plain kernels and pn_phase_taylor_ex is
refused, which the line then says).  Prints one JSON line per (strategy, stream mode): ms_other (k_pn_pixel) and ms_prepass (k_pn_chain) of every render (the
first is the warm-up), the counters of the last.  `--renders N` sets how many (default 4); under a profiler run it with `--renders 2` as the program after
`--`."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rustlight_amd import api, scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--renders", type=int, default=4)
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--g", type=float, default=None)
args = ap.parse_args()
sd = scenes.cbox_medium(1920, 1080, 0.5)
if args.g is not None:
    sd.medium = scenes.Medium(sd.medium.sigma_a, sd.medium.sigma_s, scenes.PHASE_HG, args.g)
ctx = api.Context(api.Scene(sd), 0)
seeds = api.IndependentSampler(0).block_seeds(1920, 1080)
runs = [(s, ctx.render_point_normal_taylor) for s in api.PN_TAYLOR_STRATEGIES] + [(s, ctx.render_point_normal) for s in ("eq_ex", "eq_clamped_ex", "pn_ex")]
for strategy, render in runs:
    for mode, name in ((api.STREAM_REFERENCE_ORDER, "reference"), (api.STREAM_PER_SAMPLE, "per-sample")):
        ms, pre, st = [], [], None
        try:
            for _ in range(args.renders):
                _, st = render(seeds, strategy, args.spp, True, mode)
                ms.append(round(st["ms_other"], 3)); pre.append(round(st["ms_prepass"], 3))
        except api.RustlightError as e:
            print(json.dumps({"strategy": strategy, "streams": name, "refused": e.code}), flush=True)
            continue
        keep = ("camera_samples", "rng_draws", "extension_rays", "shadow_rays", "vertices", "kernel_launches")
        print(json.dumps({"strategy": strategy, "streams": name, "g": args.g, "spp": args.spp, "ms_pixel": ms, "ms_chain": pre, **{k: st[k] for k in keep}}), flush=True)
