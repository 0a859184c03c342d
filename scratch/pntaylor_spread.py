"""The CPU figures of profiles/pntaylor_note.md for tests/test_gpu_pntaylor_quadrature.py, from tests/pntaylor_restatement.py alone (no GPU): per case
STRATEGY:MEDIUM the single-image spread of r = mean(image) / mean(quadrature) over 8 seeds at `--spp` (AA off, the test's frame and scenes), the mean of r, the
smallest power of two that puts SE(r) over 8 seeds under 2.5 % assuming 1 / sqrt(spp), and the Newton steps per inverted sample (mean, maximum); with `--teeth
STRATEGY:MEDIUM:SPP` the test's own check_ratios on the restatement's images at that spp, once as it is and once with each of pntaylor_restatement.MUTATION's two breaks;
with `--plain` the plain strategy of each case beside it (pn_restatement), for the note's comparison of spreads."""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import pn_restatement as P  # noqa: E402
from tests import pntaylor_restatement as T  # noqa: E402
from tests import test_gpu_pntaylor_quadrature as G  # noqa: E402
from tests import volume_quadrature as Q  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--spp", type=int, default=8)
ap.add_argument("--cases", default=",".join(f"{s}:{m}" for s, m in G.CASES))
ap.add_argument("--teeth", default="")
ap.add_argument("--plain", action="store_true")
args = ap.parse_args()
reference = G.PQ._Reference()
PLAIN_OF = {"eq_phase_taylor_ex": "eq_ex", "eq_tr_taylor_ex": "eq_ex", "eq_clamped_phase_taylor_ex": "eq_clamped_ex", "eq_clamped_tr_taylor_ex": "eq_clamped_ex",
            "pn_tr_taylor_ex": "pn_ex", "pn_phase_taylor_ex": "pn_ex"}


def rs_of(strategy, medium, spp, module=T):
    name, two = G.medium_of(medium)
    ref = reference.centres(name, two)
    fr = P.Frame(G.PQ._scene(name, two))
    return ref, G.ratios(ref, lambda seeds: module.render(fr, seeds, strategy, spp, False)[0])


if args.teeth:
    strategy, medium, spp = args.teeth.split(":")
    for mutation in (None, "no_prob_poly", "no_norm"):
        T.MUTATION = mutation
        ref, rs = rs_of(strategy, medium, int(spp))
        try:
            Q.check_ratios(f"{strategy} {medium} {spp} spp, {mutation or 'as it is'}", rs, ref["error"] / ref["value"])
            print("  -> passes", flush=True)
        except AssertionError as e:
            print("  -> FAILS the assertion:", str(e.args[0])[:160].replace("\n", " "), flush=True)
    sys.exit(0)
for case in args.cases.split(","):
    strategy, medium = case.split(":")
    for module, name in ((T, strategy),) + (((P, PLAIN_OF[strategy]),) if args.plain else ()):
        T.NEWTON_MAX[0] = 0
        ref, rs = rs_of(name, medium, args.spp, module)
        r = np.asarray(rs, np.float64)
        spread = r.std(axis=0, ddof=1)
        need = args.spp * (spread.max() / (0.025 * math.sqrt(G.K))) ** 2
        line = (f"{name} {medium}: spread {np.array2string(spread, precision=4)} at {args.spp} spp over {G.K} seeds, mean r {np.array2string(r.mean(axis=0), precision=4)}, "
                f"spp for SE 2.5 % {need:.2f} -> {1 << max(0, math.ceil(math.log2(max(need, 1e-9))))}")
        if module is T:
            fr = P.Frame(G.PQ._scene(*G.medium_of(medium)))
            det = T.render(fr, G.orc.block_seeds(G.CAM_SEED, G.W, G.H), name, args.spp, False)[2]
            line += f", Newton steps mean {det['newton_steps'] / max(det['took_poly'], 1):.2f} max {T.NEWTON_MAX[0]}, polynomial branch {det['took_poly']} of {det['some']}"
        print(line, flush=True)
