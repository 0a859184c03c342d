"""The CPU figures of profiles/pnats_note.md, from tests/pnats_restatement.py and tests/pn_restatement.py alone (no GPU).
Per case STRATEGY:SCENE of tests/test_gpu_pnats_quadrature.py: the single-image spread of r = mean(image) / mean(quadrature) over 8 seeds at `--spp` (AA off,
the test's frame and scenes), the mean of r, the smallest power of two that puts SE(r) over 8 seeds under 2.5 % assuming 1 / sqrt(spp), and the test's own
check_ratios on the restatement's images (`--check`: at the spp the test runs the case at).
With `--variance SPP`: the per-pixel variance over 8 seeds of eq_ex on lights8 over the tree and with the power pick (pn_restatement on the same scene without
the tree, constant emission), summed over the pixels, and their ratio — what tests/test_gpu_pnats_many_lights.py asserts on the device."""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import orc  # noqa: E402
from tests import pn_restatement as P  # noqa: E402
from tests import pnats_restatement as A  # noqa: E402
from tests import test_gpu_pnats_quadrature as G  # noqa: E402
from tests import volume_quadrature as Q  # noqa: E402
from tests.test_gpu_pnmis_quadrature import ratios  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--spp", type=int, default=8)
ap.add_argument("--cases", default=",".join(f"{s}:{m}" for s, m in G.CASES))
ap.add_argument("--check", action="store_true")
ap.add_argument("--variance", type=int, default=0)
args = ap.parse_args()

if args.variance:
    sd = A.scene("lights8_const", G.W, G.H)
    plain = A.lights(8, G.W, G.H, hsv=False, use_ats=False)
    fa, fp = A.Frame(sd), P.Frame(plain)
    imgs = {"tree": [], "power": []}
    for k in range(G.K):
        seeds = orc.block_seeds(G.CAM_SEED + k, G.W, G.H)
        imgs["tree"].append(A.render(fa, seeds, "eq_ex", args.variance)[0])
        imgs["power"].append(P.render(fp, seeds, "eq_ex", args.variance)[0])
    var = {k: np.asarray(v, np.float64).var(axis=0, ddof=1).sum(axis=(0, 1)) for k, v in imgs.items()}
    mean = {k: np.asarray(v, np.float64).mean(axis=(0, 1, 2)) for k, v in imgs.items()}
    print(f"eq_ex lights8 at {args.variance} spp over {G.K} seeds: summed per-pixel variance tree {var['tree']}, power {var['power']}, ratio {var['tree'] / var['power']}")
    print(f"  image means tree {mean['tree']}, power {mean['power']}")
    sys.exit(0)
reference = G._Reference()
for case in args.cases.split(","):
    strategy, name = case.split(":")
    spp = G.SPP[(strategy, name)] if args.check else args.spp
    ref = reference.centres(name)
    fr = A.Frame(G.scene(name))
    rs = ratios(ref, lambda seeds: A.render(fr, seeds, strategy, spp, False)[0])
    r = np.asarray(rs, np.float64)
    spread = r.std(axis=0, ddof=1)
    need = spp * (spread.max() / (0.025 * math.sqrt(G.K))) ** 2
    print(f"{strategy} {name}: spread {np.array2string(spread, precision=4)} at {spp} spp over {G.K} seeds, mean r {np.array2string(r.mean(axis=0), precision=4)}, "
          f"spp for SE 2.5 % {need:.2f} -> {1 << max(0, math.ceil(math.log2(max(need, 1e-9))))}", flush=True)
    if args.check:
        try:
            Q.check_ratios(f"{strategy} {name} {spp} spp", rs, ref["error"] / ref["value"])
            print("  -> passes", flush=True)
        except AssertionError as e:
            print("  -> FAILS the assertion:", str(e.args[0])[:200].replace("\n", " "), flush=True)
