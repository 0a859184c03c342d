"""Light-path generation on per-path sampler streams (rl_vpl_generate_paths, kernels/vpl_paths.hip.h) restated from entry points the oracle already has, the
yardstick of tests/test_vpl_paths_restatement.py and tests/test_gpu_vpl_paths_exact.py (a plain module: `from tests import vpl_paths_restatement`).

The contract: light path k draws from orc.Rng(seed_k, variant), seed_k the k-th next_u64() of the main sampler; paths are shot while fewer than nb records are
stored.  One path of the serial pass is Scene.vpl_generate(state, nb_vpl = 1, .., VPL_ALL): with VPL_ALL the light vertex always stores a record, so nb_vpl = 1
shoots exactly one path (asserted on every call), and option_vpl only gates stores and never draws, so any option's records are a filter of the VPL_ALL records
by their kind word."""
import numpy as np

from oracle import orc
from rustlight_amd import abi, api

KIND_VOLUME = 1                   # RL_VPL_KIND_VOLUME, word 0 of a record
GEN_KEYS = ("vertices", "extension_rays", "rng_draws")


def keep(records, option_vpl):
    """The records of one path that option_vpl stores."""
    if option_vpl == api.VPL_ALL:
        return records
    volume = records[:, 0] == KIND_VOLUME
    return records[volume] if option_vpl == api.VPL_VOLUME else records[~volume]


def generate(sc, state, nb_vpl, max_depth=None, rr_depth=0, option_vpl=api.VPL_ALL, seed_variant=0):
    """sc: orc.Scene; state: the main sampler's four words.  {"records" [n, 24] u32, "n_paths" = K, "state" after (advanced by K next_u64), "gen_stats"
    {camera_samples, vertices, extension_rays, rng_draws} summed over the K paths, "per_path" [K, 4] = records kept, vertices, extension rays, draws}."""
    main = orc.Rng.from_state([int(v) for v in state])
    kept, per_path = [], []
    stored = 0
    while stored < nb_vpl:
        assert len(per_path) < orc.VPL_MAX_PATHS, "generation did not end"
        r = orc.Rng(main.next_u64(), seed_variant)
        rec, n, _, st = sc.vpl_generate(r.state, 1, max_depth, rr_depth, orc.VPL_ALL)
        assert n == 1
        rec = keep(rec, option_vpl)
        kept.append(rec.copy())
        stored += rec.shape[0]
        per_path.append([rec.shape[0]] + [st[k] for k in GEN_KEYS])
    per_path = np.asarray(per_path, np.uint64).reshape(-1, 4)
    stats = {"camera_samples": len(kept)}
    for i, k in enumerate(GEN_KEYS):
        stats[k] = int(per_path[:, 1 + i].sum())
    return {"records": np.concatenate(kept, axis=0), "n_paths": len(kept), "state": np.array(list(main.state), np.uint64), "gen_stats": stats, "per_path": per_path}


def block_seeds_after(sd, state):
    """The block seeds drawn from the sampler a generation left."""
    st = np.array(state, np.uint64).copy()
    seeds = np.zeros(orc.lib().orc_block_count(sd.width, sd.height), np.uint64)
    orc.lib().orc_generate_block_seeds(abi.u64ptr(st), sd.width, sd.height, abi.u64ptr(seeds))
    return seeds


def compute(sd, seed=0, nb_vpl=128, max_depth=None, rr_depth=0, option_vpl=api.VPL_ALL, seed_variant=0):
    """The generation from `-r independent:SEED` and the block seeds of the advanced sampler; "scene" is the orc.Scene for what follows (render_vpl, the BRE)."""
    sc = orc.Scene(sd)
    ref = generate(sc, orc.Rng(seed, seed_variant).state, nb_vpl, max_depth, rr_depth, option_vpl, seed_variant)
    ref["seeds"] = block_seeds_after(sd, ref["state"])
    ref["scene"] = sc
    return ref


# ---- the fixtures both test files lean on: (frame, nb, option, max_depth, rr_depth) on cbox_medium(w, h, 1.0), seed 3
FIXTURES = {
    "volume": ((32, 24), 300, api.VPL_VOLUME, None, 0),
    "all": ((32, 24), 300, api.VPL_ALL, None, 0),
    "surface": ((32, 24), 300, api.VPL_SURFACE, None, 0),
    "depth3": ((24, 16), 100, api.VPL_VOLUME, 3, 2),        # some paths store nothing; K is several batches of 7 and no multiple of 7
    "one_path": ((24, 16), 5, api.VPL_VOLUME, None, 0),     # K = 1: the single path's records are all kept
    "many_paths": ((32, 24), 12500, api.VPL_SURFACE, None, 0),     # K is past the first default batch of 4096 paths: kept paths reach their seed through the jump table
}
FIXTURE_SEED = 3
FORCED_BATCH = 7
FIRST_DEFAULT_BATCH = 4096          # the host's first batch when nb_vpl / 8 is smaller

_cache = {}


def fixture(name):
    """(scene description, the restatement's result) of a fixture, computed once per process and not to be modified."""
    if name not in _cache:
        from rustlight_amd import scenes
        (w, h), nb, option, max_depth, rr_depth = FIXTURES[name]
        sd = scenes.cbox_medium(w, h, 1.0)
        _cache[name] = (sd, compute(sd, FIXTURE_SEED, nb, max_depth, rr_depth, option))
    return _cache[name]
