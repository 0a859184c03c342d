"""The CPU figures of profiles/pnmis_note.md for tests/test_gpu_pnmis_quadrature.py, from tests/pnmis_restatement.py alone (no GPU): per case the
single-image spread of r = mean(image) / mean(quadrature) over 8 seeds at `--spp` (AA off, the test's frame and scenes), and the smallest power of two that
puts SE(r) over 8 seeds under 2.5 % assuming 1 / sqrt(spp); with `--teeth FAMILY:MEDIUM:SPP` the test's own check_ratios on the restatement's images at that
spp, once as it is and once with each of pnmis_restatement.MUTATION's three breaks."""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import pnmis_restatement as M  # noqa: E402
from tests import test_gpu_pnmis_quadrature as T  # noqa: E402
from tests import volume_quadrature as Q  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--cases", default="tr:grey,eq:grey,clamped:grey,pn:grey,eq:coloured,pn:coloured,eq:two,clamped:two,pn:two")
ap.add_argument("--teeth", default="")
args = ap.parse_args()
reference = T._Reference()


def rs_of(fam, medium, spp):
    two = medium == "two"
    name = "grey" if two else medium
    ref = reference.centres(name, two)
    fr = M.Frame(T._scene(name, two))
    return ref, T.ratios(ref, lambda seeds: M.render(fr, seeds, T.ONE_NAME[fam], spp, False)[0])


if args.teeth:
    fam, medium, spp = args.teeth.split(":")
    for mutation in (None, "no_sigma_s", "no_inv_pdf", "weight_one"):
        M.MUTATION = mutation
        ref, rs = rs_of(fam, medium, int(spp))
        try:
            Q.check_ratios(f"{fam} {medium} {spp} spp, {mutation or 'as it is'}", rs, ref["error"] / ref["value"])
            print("  -> passes", flush=True)
        except AssertionError as e:
            print("  -> FAILS the assertion:", str(e.args[0])[:160].replace("\n", " "), flush=True)
    sys.exit(0)
for case in args.cases.split(","):
    fam, medium = case.split(":")
    ref, rs = rs_of(fam, medium, args.spp)
    r = np.asarray(rs, np.float64)
    spread = r.std(axis=0, ddof=1)
    need = args.spp * (spread.max() / (0.025 * math.sqrt(T.K))) ** 2
    print(f"{fam} {medium}: spread {np.array2string(spread, precision=4)} at {args.spp} spp over {T.K} seeds, mean r {np.array2string(r.mean(axis=0), precision=4)}, "
          f"spp for SE 2.5 % {need:.2f} -> {1 << max(0, math.ceil(math.log2(max(need, 1e-9))))}", flush=True)
