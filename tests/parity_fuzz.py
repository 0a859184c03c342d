"""Randomized differential test, HIP path vs CPU oracle (bit-exact image + counters), over random scene / light / material /
integrator-option / pipeline combinations.  `run(seconds, seed)` is used by tests/test_gpu_parity.py (short) and can be run by hand
for longer: python tests/parity_fuzz.py [seconds] [seed] [fast | light | stratified]   (round 1: ~75 000 cases over eight runs on 1 x MI355X, 0 failures; round 2: 26 k + 17 k + 17 k + 34 k + 69 k + 87 k cases, the last four with a third of the
cases forced through the kernels that stream the BVH, 0 mismatches).
`fast`: eligible cases are also rendered with the opt-in tolerance build (`numerics = fast`) and held to a statistical bar (vertex
count within 2 % of the exact build at the same seeds — the path census is what a systematic error moves —, image mean within a coarse bound)."""
import os, sys, time, traceback
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from rustlight_amd import api, scenes
from oracle import orc
S = scenes


def run(budget=20.0, seed=0, verbose=True, fast=False, arm="path"):
    """arm: "path" (path / ao / direct in their random stream modes), "light" (the light tracer, rl_render_light, on the scenes without an
    environment emitter) or "stratified" (path / ao / direct with RL_STREAM_STRATIFIED)."""
    rng = np.random.default_rng(seed)
    def rand_color(lo=0.05, hi=0.9):
        return tuple(float(x) for x in rng.uniform(lo, hi, 3))

    def rand_bsdf():
        k = rng.integers(0, 9)
        tex = lambda: ({"type": S.TEX_CHECKERBOARD, "color0": rand_color(), "color1": rand_color(), "scale": (float(rng.uniform(1, 6)), float(rng.uniform(1, 6)))}
                       if rng.random() < 0.3 else S.const_color(rand_color()))
        if k <= 2: return S.Bsdf(type=S.DIFFUSE, diffuse=tex())
        if k == 3: return S.Bsdf(type=S.PHONG, diffuse=tex(), specular=S.const_color(rand_color(0.05, 0.5)), exponent=float(rng.uniform(2, 80)), weight_specular=float(rng.uniform(0.1, 0.9)))
        if k == 4: return S.Bsdf(type=S.METAL, distribution=S.MF_NONE)
        if k == 5: return S.Bsdf(type=S.METAL, distribution=int(rng.choice([S.MF_BECKMANN, S.MF_GGX])), alpha_u=float(rng.uniform(0.05, 0.6)), alpha_v=float(rng.uniform(0.05, 0.6)))
        if k == 6: return S.Bsdf(type=S.GLASS)
        return S.Bsdf(type=S.SUBSTRATE, diffuse=tex(), specular=S.const_color(rand_color(0.02, 0.1)), distribution=int(rng.choice([S.MF_NONE, S.MF_GGX, S.MF_BECKMANN])),
                      alpha_u=float(rng.uniform(0.05, 0.5)), alpha_v=float(rng.uniform(0.05, 0.5)))

    def rand_scene():
        w, h = int(rng.integers(5, 49)), int(rng.integers(5, 41))
        kind = rng.integers(0, 6)
        if kind == 0: sd = S.cbox(w, h)
        elif kind == 1: sd = S.cbox_other_lights(w, h, point=bool(rng.integers(2)), directional=bool(rng.integers(2)), environment=bool(rng.integers(2)), keep_area_light=bool(rng.integers(2)))
        elif kind == 2: sd = S.sky_scene(w, h, keep_area_light=bool(rng.integers(2)))
        elif kind == 3: sd = S.many_lights(w, h, n=int(rng.integers(2, 5)), use_ats=bool(rng.integers(2)), glowing_spheres=int(rng.integers(0, 3)))
        elif kind == 4: sd = S.living_room(w, h, n_spheres=int(rng.choice([8, 27])), tess=int(rng.integers(4, 12)))
        else: sd = S.cbox_medium(w, h, float(rng.uniform(0.1, 1.0)), float(rng.uniform(0.0, 0.3)), g=float(rng.choice([0.0, 0.5, -0.3])))
        if kind != 4 and rng.random() < 0.6:
            for m in sd.meshes:
                if m.emission is None and rng.random() < 0.5: m.bsdf = rand_bsdf()
        if kind in (0, 1, 3) and rng.random() < 0.2:
            sd.medium = S.Medium(rand_color(0.0, 0.2), rand_color(0.1, 0.8), int(rng.choice([S.PHASE_ISOTROPIC, S.PHASE_HG])), float(rng.uniform(-0.6, 0.6)))
            sd.environment = None; sd.environment_map = None      # (no environment with a medium)
        # `-x hvs-light` / `-x texture-light` (cli.rs:410-429): the light meshes' emission becomes uv-dependent (EmissionType::HSV / Texture) — when they all carry uv
        lights = [m for m in sd.meshes if m.emission is not None]
        if lights and all(m.uv is not None for m in lights) and rng.random() < 0.15:
            kind_e = "hsv" if rng.random() < 0.5 else "texture"
            bid = -1
            if kind_e == "texture":
                tw, th = int(rng.integers(1, 6)), int(rng.integers(1, 6))
                sd.bitmaps.append((tw, th, rng.uniform(0.0, 3.0, (tw * th, 3)).astype(np.float32)))
                bid = len(sd.bitmaps) - 1
            S.override_light_emission(sd, kind_e, bitmap_id=bid)
        return sd

    def rand_params(sd):
        has_emitter = any(m.emission for m in sd.meshes) or bool(sd.lights) or sd.environment is not None or getattr(sd, "environment_map", None) is not None
        kw = dict(spp=int(rng.integers(1, 6)))
        kw["max_depth"] = None if rng.random() < 0.2 else int(rng.integers(0, 12))
        kw["min_depth"] = None if rng.random() < 0.6 else int(rng.integers(0, 6))
        kw["rr_depth"] = None if rng.random() < 0.2 else int(rng.integers(0, 5))
        kw["strategy"] = int(rng.choice([api.STRATEGY_ALL, api.STRATEGY_BSDF, api.STRATEGY_EMITTER])) if has_emitter else api.STRATEGY_BSDF
        kw["single_scattering"] = bool(rng.random() < 0.15)
        kw["stream_mode"] = int(rng.choice([api.STREAM_PER_SAMPLE, api.STREAM_PER_SAMPLE, api.STREAM_REFERENCE_ORDER]))
        kw["seed_variant"] = int(rng.integers(0, 2))
        if kw["max_depth"] is None and kw["rr_depth"] is None: kw["rr_depth"] = 2      # keep paths finite
        if rng.random() < 0.25:                                                        # one shard of a tile-sharded render
            kw["shard_count"] = int(rng.integers(2, 5)); kw["shard_index"] = int(rng.integers(0, kw["shard_count"]))
        return kw

    t_end = time.time() + budget
    n = bad = n_fast = 0
    while time.time() < t_end:
        state = rng.bit_generator.state
        try:
            sd = rand_scene()
            kw = rand_params(sd)
            seed = int(rng.integers(0, 1000))
            pipe = int(rng.choice([0, 1, 2])); split = int(rng.choice([0, 0, 1, 2, 3])); pool = int(rng.choice([0, 0, 512, 4096])) if pipe != 2 else 0
            # a third of the cases run the kernels that stream the BVH from L2 / HBM (wave-voted trips, scalar-cache fetches, stack overflow to global
            # memory) instead of the LDS-staged ones small scenes would get
            streaming = rng.random() < 0.33
            if streaming: os.environ["RL_FORCE_STREAMING"] = "1"
            try:
                ctx, osc = api.Context(api.Scene(sd), 0), orc.Scene(sd)
            finally:
                os.environ.pop("RL_FORCE_STREAMING", None)
            if arm == "light":        # IntegratorLightTracing: every random scene but those with an environment emitter (rl_render_light refuses them)
                if sd.environment is not None or getattr(sd, "environment_map", None) is not None or not (any(m.emission for m in sd.meshes) or sd.lights):
                    continue
                lk = dict(spp=kw["spp"], min_depth=kw["min_depth"], max_depth=kw["max_depth"], rr_depth=kw["rr_depth"], strategy=int(rng.integers(0, 3)),
                          seed_variant=kw["seed_variant"])
                seeds = api.IndependentSampler(seed, kw["seed_variant"]).block_seeds(sd.width, sd.height)
                img, st = ctx.render_light(seeds, **lk); ref, ost = osc.render_light(seeds=seeds, **lk)
                keys = ("camera_samples", "vertices", "extension_rays", "shadow_rays", "rng_draws", "splats", "splats_invalid", "splats_saturated")
                n += 1
                if not (np.array_equal(img, ref) and all(st[k] == ost[k] for k in keys)):
                    bad += 1
                    print("MISMATCH (light)", n, dict(size=(sd.width, sd.height), tris=sd.n_triangles, streaming=streaming, seed=seed, **lk),
                          "max abs diff", float(np.nanmax(np.abs(img - ref))), {k: (st[k], ost[k]) for k in keys}, flush=True)
                continue
            if arm == "stratified":
                kw["stream_mode"] = api.STREAM_STRATIFIED
            which = rng.random()
            if which < 0.25:          # the `ao` / `direct` integrators (no medium there: src/integrators/{ao,direct}.rs ignore it)
                seeds = api.IndependentSampler(seed, kw["seed_variant"]).block_seeds(sd.width, sd.height)
                mk = dict(spp=kw["spp"], stream_mode=kw["stream_mode"], seed_variant=kw["seed_variant"], shard_index=kw.get("shard_index", 0), shard_count=kw.get("shard_count", 1))
                has_emitter = any(m.emission for m in sd.meshes) or bool(sd.lights) or sd.environment is not None or getattr(sd, "environment_map", None) is not None
                if which < 0.1 or not has_emitter:
                    mk.update(max_distance=None if rng.random() < 0.3 else float(rng.uniform(0.1, 2.0)), normal_correction=bool(rng.integers(2)))
                    img, st = ctx.render_ao(seeds, **mk); ref, ost = osc.render_ao(seeds=seeds, **mk)
                    keys = ("camera_samples", "extension_rays", "rng_draws")
                else:
                    nb, nl = int(rng.integers(0, 4)), int(rng.integers(0, 4))
                    if nb + nl == 0: nl = 1
                    mk.update(nb_bsdf_samples=nb, nb_light_samples=nl)
                    img, st = ctx.render_direct(seeds, **mk); ref, ost = osc.render_direct(seeds=seeds, **mk)
                    keys = ("camera_samples", "extension_rays", "shadow_rays", "rng_draws")
                n += 1
                if not (np.array_equal(img, ref) and all(st[k] == ost[k] for k in keys)):
                    bad += 1
                    print("MISMATCH (ao/direct)", n, dict(size=(sd.width, sd.height), tris=sd.n_triangles, streaming=streaming, seed=seed, **mk), "max abs diff", float(np.nanmax(np.abs(img - ref))), flush=True)
                continue
            # reference-order streams through the persistent kernel: half of the cases through the speculative chain pass (k_stream_spec, forced — these
            # renders are far too small for it to be chosen) with random lanes per block / per pixel, track capacities, window margins and lead-ins
            spec_env = {}
            if kw["stream_mode"] == api.STREAM_REFERENCE_ORDER and pipe != 1 and pool == 0 and rng.random() < 0.5:
                g = int(rng.choice([16, 32, 64, 256]))
                spec_env = dict(RL_SPEC_FORCE="1", RL_SPEC_GROUP=str(g), RL_SPEC_SUB=str(int(rng.choice([s for s in (1, 2, 4, 8, 16) if s <= g]))), RL_SPEC_EXTRA=str(int(rng.integers(2))), RL_SPEC_PROBE_EVERY=str(int(rng.random() < 0.2)),
                                RL_SPEC_CAP=str(int(rng.choice([4, 9, 40, 400]))), RL_SPEC_LEAD=str(int(rng.choice([0, 2, 24]))),
                                RL_SPEC_KS=str(float(rng.choice([0.0, 1.65, 4.0]))), RL_SPEC_KE=str(float(rng.choice([0.0, 1.65, 4.0]))), RL_SPEC_PROBE=str(int(rng.choice([0, 3, 32]))),
                                RL_SPEC_DENSE=str(int(rng.choice([0, 2, 5, 16, 64]))), RL_SPEC_DENSE_FRAC=str(float(rng.choice([0.0, 0.3, 0.6, 0.9]))))      # (serial walks on the group's idle lanes)
                if rng.random() < 0.2: spec_env["RL_SPEC_NO_TRIVIAL"] = "1"
                if rng.random() < 0.2: spec_env["RL_STATE_BUDGET_MB"] = "1"
            with ctx.options(**{k[3:].lower(): v for k, v in spec_env.items()}):      # (rl_context_set_option: the render path never reads the environment)
                img, st = ctx.render(api.IndependentSampler(seed, kw["seed_variant"]).block_seeds(sd.width, sd.height), api.path_params(pipeline=pipe, sample_split=split, pool_slots=pool, **kw))
            if spec_env: kw = dict(kw, _spec=spec_env)
            ref, ost = osc.render(master_seed=seed, eval_order=1, **{k: v for k, v in kw.items() if k != "_spec"})
            ok = np.array_equal(img, ref) and all(st[k] == ost[k] for k in ("camera_samples", "vertices", "extension_rays", "rng_draws", "shadow_rays"))
            n += 1
            if ok and fast and pipe != 1 and pool == 0 and kw["stream_mode"] == api.STREAM_PER_SAMPLE:
                # the opt-in tolerance build on the same case, at more samples: same seeds, so all but the paths whose decisions flip (a fraction
                # of a percent) are the same paths.  The robust signal of a systematic error is the path census — the contraction trap that once
                # blackened guarded colour products moved the vertex count by 10 % — so that is held to 2 % (+ 64 vertices; the widest of 12 764 tolerance-build cases on the final round-2 tree moved it by 1.4 %); the image mean of these tiny,
                # often high-variance renders (min_depth, BSDF-only strategy: a single flipped light hit moves it by percents; 16 of 2608 cases
                # moved it by more than 2 % in a 6-minute run, none by more than 40 %, all with vertex counts within 0.6 %) only to a coarse bound
                # (a handful of flipped paths can also be hundreds of vertices long — glass, min_depth — and move the census of a tiny render by several percent
                # while the image stays put: 2 of 4230 cases, per-pixel L2 1e-16; those pass on the image)
                kf = dict({k: v for k, v in kw.items() if k != "_spec"}, spp=max(32, 8 * kw["spp"]))
                seeds = api.IndependentSampler(seed, kw["seed_variant"]).block_seeds(sd.width, sd.height)
                ex, sx = ctx.render(seeds, api.path_params(pipeline=pipe, sample_split=split, **kf))
                fa, sf = ctx.render(seeds, api.path_params(pipeline=pipe, sample_split=split, numerics=api.NUMERICS_FAST, **kf))
                n_fast += 1
                mx, mf = float(np.mean(ex, dtype=np.float64)), float(np.mean(fa, dtype=np.float64))
                e = np.sum((ex.astype(np.float64) - fa) ** 2, -1)
                fine = (np.isfinite(fa).all() or not np.isfinite(ex).all()) and (sx["camera_samples"] < 20000 or abs(mf - mx) <= 0.5 * abs(mx) + 1e-3) and (abs(sf["vertices"] - sx["vertices"]) <= 0.02 * sx["vertices"] + 64 or float(e.mean()) <= 1e-9)
                if not fine:
                    bad += 1
                    print("FAST-MODE DRIFT", n, dict(size=(sd.width, sd.height), meshes=len(sd.meshes), tris=sd.n_triangles, pipe=pipe, split=split, seed=seed, **kf),
                          "means", mx, mf, "vertices", sx["vertices"], sf["vertices"], "L2 mean", float(e.mean()), flush=True)
            if not ok:
                bad += 1
                print("MISMATCH", n, dict(size=(sd.width, sd.height), meshes=len(sd.meshes), tris=sd.n_triangles, streaming=streaming, pipe=pipe, split=split, pool=pool, seed=seed, **kw),
                      "max abs diff", float(np.nanmax(np.abs(img - ref))), {k: (st[k], ost[k]) for k in ("vertices", "rng_draws", "shadow_rays")}, flush=True)
        except Exception as e:
            bad += 1
            print("ERROR", n, repr(e), flush=True); traceback.print_exc()
    if verbose:
        print(f"fuzz: {n} cases ({n_fast} also through numerics = fast), {bad} failures", flush=True)
    return n, bad


if __name__ == "__main__":
    arms = [a for a in ("light", "stratified") if a in sys.argv[3:]]
    n, bad = run(float(sys.argv[1]) if len(sys.argv) > 1 else 120.0, int(sys.argv[2]) if len(sys.argv) > 2 else 0, fast="fast" in sys.argv[3:],
                 arm=arms[0] if arms else "path")
    sys.exit(1 if bad else 0)
