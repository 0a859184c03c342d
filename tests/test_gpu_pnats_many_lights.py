"""What the light tree is for: on lights8 (tests/pnats_restatement.py: eight small quads, most of which cannot reach a given camera ray, or reach it
weakly) at equal spp over K = 8 seeds, the per-pixel variance of eq_ex with the emitter picked from the tree by the ray importance is below that of
`point-normal -s eq_ex` on the same scene without the tree, where the emitter is picked by power.  The assertion is only "lower"; profiles/pnats_note.md has
the ratio measured on the device and the one the restatements give on the CPU (scratch/pnats_spread.py --variance)."""
import numpy as np
import pytest

from oracle import orc
from tests import pnats_restatement as A
from tests.scene_helpers import context as _context

pytestmark = pytest.mark.gpu

W, H, K, SPP, CAM_SEED = 24, 18, 8, 4, 4000


def test_the_tree_lowers_the_variance_of_eq_ex(built):
    tree = _context(A.scene("lights8", W, H))
    power = _context(A.lights(8, W, H, use_ats=False))
    a, b = [], []
    for k in range(K):
        seeds = orc.block_seeds(CAM_SEED + k, W, H)
        a.append(tree.render_point_normal_ats(seeds, "eq_ex", SPP)[0])
        b.append(power.render_point_normal(seeds, "eq_ex", SPP)[0])
    var_tree = np.asarray(a, np.float64).var(axis=0, ddof=1).sum(axis=(0, 1))
    var_power = np.asarray(b, np.float64).var(axis=0, ddof=1).sum(axis=(0, 1))
    print(f"summed per-pixel variance of eq_ex on lights8 at {SPP} spp over {K} seeds: tree {var_tree}, power {var_power}, ratio {var_tree / var_power}")
    assert np.all(var_tree < var_power), (var_tree, var_power)
