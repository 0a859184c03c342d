#!/usr/bin/env python
"""bench.py — Msamples/s of the `path` hot path on BASELINE.json configs[1]:
cbox, 1920x1080, 128 spp per GPU, diffuse-only, per-sample stream mode, N x MI355X (pixel-tile shards +
one RCCL framebuffer reduce).  One "step" = one full render (W*H*spp camera samples).

Timed region: rl_render_path (tile seeding -> kernels -> framebuffer in HBM) + the RCCL reduce
(N > 1) + the framebuffer download to pinned host memory on rank 0.  Scene construction, BVH build and upload are
outside, as in the reference (integrators/mod.rs:280 vs 324-334).

`python bench.py --gpus N` starts its own N ranks (re-executes itself under torch.distributed.run) unless it already runs
under a launcher (WORLD_SIZE set).  On a box with fewer GPUs than ranks the ranks share devices and the reduce goes
through gloo — a plumbing mode, flagged in the JSON (`devices_shared`), never a scaling measurement.
`--scaling weak` (default): the image is fixed and spp = 128 x N, every GPU traces W*H*128 camera samples per step (N = 8 is
BASELINE configs[3]); `--scaling strong`: 128 spp in total, the tiles split N ways.

Prints ONE JSON line (rank 0).  A plain run does only what the headline needs: it sets up, warms up, times the steps, writes
--dump-outputs and prints the line, whose `roofline` is for the dominant kernel (k_path_fused on this workload): algorithmic bytes
per launch / mean launch duration from HIP events on the render stream of the timed steps themselves.  Everything else needs `--full`
(`full` in the line says which it was; extras() lists the parts): `oracle_crc_match` (the last frame against the CPU oracle's CRC of it),
`cpu_baseline`, which times the CPU oracle (a C++ restatement of rustlight's path integrator — NOT rustlight itself) on a bounded
sample of the same workload on the host cores, the N-GPU records below, and `also`: on the default single-GPU run the other BASELINE
configurations and stream modes timed the same way in the same process (configs[2] stand-in, configs[4], configs[1] in
rustlight's own reference-order streams, configs[1] on a square frame), and `reference_order_value` at the top level.
`value`, `reference_order_value` and every `ms_per_step` are ONE frame at a time (rl_render_path is synchronous, like Integrator::compute).  Next to
them, never in their place: `reference_order_in_flight_value` and the `*_3_in_flight` records — the same frames with three of them on the GPU at once
(three contexts of the scene, one host thread each; DESIGN.md 5 "Frames in flight") — and, for N > 1, `reference_order.three_frames_in_flight` per rank
(the N-GPU records of --full: `reference_order`, `strong_scaling`, and `distributed.crc_match` from a single-GPU re-render of the last frame).
The reference-order `also` records (configs[1], configs[4], the configs[2] stand-in in rustlight's own streams: the drop-in default) are THREE timed steps each, every step
synchronised and timed on its own: `step_ms`, `value_min` (the worst single step) / `value_median` / `value_max`, and `reference_order_worst_step_value` at the top level = the
weakest step of the default mode over all three.  In that mode k_path_fused runs BESIDE the chain pass: its `kernel_ms` / roofline entry use its own span
(rl_render_stats.ms_eval_span), `eval_tail_after_chain_ms` is what of it was left after the chain pass had ended."""
from __future__ import annotations

import argparse
import datetime
import json
import os
import socket
import sys
import threading
import time
import zlib

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# multi-process GPU work on this pool needs dmabuf IPC; the runtime reads this when it initialises, i.e. before the first torch.cuda call
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np  # noqa: E402

PEAK_HBM_GBPS = 8000.0


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=128, help="samples per pixel PER GPU (weak scaling: the render uses spp x N)")
    ap.add_argument("--scene", default="cbox", choices=["cbox", "cbox_medium", "living_room"])
    ap.add_argument("--tris", type=int, default=0, help="living_room only: tessellate the spheres finer until the scene has at least this many triangles "
                    "(SURVEY 8(d): >= 4 M puts nodes + triangles past the 256 MB Infinity Cache)")
    ap.add_argument("--pool", type=int, default=0)
    ap.add_argument("--pipeline", default="auto", choices=["auto", "wavefront", "fused"])
    ap.add_argument("--stream-mode", default="per_sample", choices=["per_sample", "reference"],
                    help="per_sample: one lane per pixel / sample (throughput decomposition); reference: rustlight's own stream assignment (one sampler per 16x16 block)")
    ap.add_argument("--numerics", default="exact", choices=["exact", "fast"])
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"], help="weak: spp x N (fixed work per GPU); strong: spp in total, tiles split N ways")
    ap.add_argument("--full", action="store_true", help="also measure and check what the headline does not need (see extras()): the CPU baseline, the `also` records, "
                    "N > 1: the reference-order / frames-in-flight / strong-scaling records and the single-GPU re-render of the last frame, and the oracle CRC comparisons. "
                    "Without it a run sets up, warms up, times the steps, writes --dump-outputs and prints the line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-verify", action="store_true", help="with --full: skip the untimed single-GPU re-render that checks the N-GPU image CRC")
    ap.add_argument("--no-also", action="store_true", help="with --full: skip the `also` sub-records (the other BASELINE configs / stream modes) of the default single-GPU run "
                    "and the reference-order / strong-scaling records of an N-GPU run")
    ap.add_argument("--init-timeout", type=float, default=180.0, help="seconds the process-group init and the first collective may take before the rank prints diagnostics and exits")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write the image the last timed step produced (rank 0: the reduced frame) "
                    "as DIR/image.npy (float32, H x W x 3); past 64 MB, a fixed seeded sample of its pixels instead (image_sample.npy + image_sample_index.npy)")
    return ap.parse_args(argv)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _respawn_under_launcher(args):
    """`python bench.py --gpus N` without a launcher: become `python -m torch.distributed.run ... bench.py <same args>`."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__), *sys.argv[1:]]
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.setdefault("OMP_NUM_THREADS", "4")
    sys.stdout.flush()
    os.execvp(cmd[0], cmd)


def is_default_workload(args) -> bool:
    """The driver's workload (`python bench.py --gpus 1 ...`): BASELINE configs[1] untouched — only on it (and with --full) the `also` records are added."""
    return (args.gpus == 1 and args.scene == "cbox" and (args.width, args.height, args.spp) == (1920, 1080, 128) and args.stream_mode == "per_sample"
            and args.numerics == "exact" and args.pipeline == "auto" and args.pool == 0 and args.tris == 0 and not args.no_also)


def extras(args) -> dict:
    """What a run does besides its headline (set-up, warm-up, the timed steps, --dump-outputs, the line with its roofline from those steps' own counters).
    All of it needs --full: a plain run is what the driver repeats, and these cost seconds to minutes of GPU and CPU time apiece."""
    multi = args.gpus > 1 and args.scene == "cbox" and args.stream_mode == "per_sample" and args.numerics == "exact" and not args.no_also
    return {"also": args.full and is_default_workload(args),                                       # the other configs / stream modes, frames in flight
            "cpu_baseline": args.full and args.gpus == 1 and not args.no_cpu_baseline,            # the CPU oracle on a bounded sample of the workload
            "reference_order": args.full and multi,                                               # N > 1: the shards in reference-order streams, 3 frames in flight
            "strong_scaling": args.full and multi and args.scaling == "weak",                     # N > 1: the strong-scaling pair of the same frame
            "verify": args.full and args.gpus > 1 and not args.no_verify,                         # N > 1: the last frame re-rendered on one GPU, CRCs compared
            "oracle_crc": args.full}                                                              # the last frame's CRC against tests/golden/bench_crcs.json


class _Watchdog:
    """A collective that never returns (first RCCL contact between ranks: peer access, IPC handles, a wrong device) must not hang the
    driver's run silently: after `seconds` the rank prints who / where it is and exits non-zero."""

    def __init__(self, what, seconds, info):
        self.t = threading.Timer(seconds, self._fire)
        self.what, self.info, self.seconds = what, info, seconds
        self.t.daemon = True

    def _fire(self):
        print(f"bench.py: {self.what} did not finish within {self.seconds:.0f} s: {json.dumps(self.info)}", file=sys.stderr, flush=True)
        os._exit(3)

    def __enter__(self):
        self.t.start()
        return self

    def __exit__(self, *exc):
        self.t.cancel()
        return False


def oracle_crc(workload, width, height, spp, stream_mode, seed):
    """CRC-32 the parity build of the CPU oracle gave for this frame (tests/golden/bench_crcs.json, made by tests/golden/make_bench_golden.py in the build
    container) — a table lookup: the timed program neither imports nor runs the oracle for this.  None when the frame is not in the table."""
    try:
        table = json.load(open(os.path.join(ROOT, "tests", "golden", "bench_crcs.json")))
    except (OSError, ValueError):
        return None
    e = table.get(f"{workload}:{width}x{height}x{spp}:{stream_mode}:seed{seed}")
    return e["crc32"] if e else None


def utilisation_fields(live, key, kernel, src_hash):
    """The honest utilisation next to the nominal `frac`: from the counter summary of profiles/pmc_live.json for this workload — VALU issue slots
    busy (SQ_INSTS_VALU x calibrated cycles per wave64 instruction / SIMD cycles), live lanes per issued VALU instruction (SQ_THREAD_CYCLES_VALU / 64 SQ_ACTIVE_INST_VALU)
    and their product = the share of the chip's FP32 lane-slots doing work.  None when no entry exists for this workload and kernel; `pmc_current` says whether the
    counters were collected on the kernel sources this run uses."""
    e = (live or {}).get(key)
    if not e or e.get("kernel") != kernel:
        return None
    busy = (e.get("valu_issue_model") or {}).get("valu_issue_busy")
    lanes = e.get("lane_utilisation")
    return {"valu_issue_busy": busy, "lane_utilisation": lanes, "valu_lane_slots_used": (busy * lanes) if (busy is not None and lanes is not None) else None,
            "wave_time_waiting": (e.get("wave_time_shares") or {}).get("SQ_WAIT_ANY"), "l2_hit_rate": e.get("l2_hit_rate"), "hbm_bytes_per_launch": e.get("hbm_bytes_per_launch"),
            "kernel_ms_under_profiler": e.get("kernel_ms_under_profiler"), "pmc_current": e.get("kernel_src_hash") == src_hash, "pmc_commit": e.get("commit")}


def pipeline_bytes(stats_sum, pixels, steps):
    """SURVEY.md §8(d) / DESIGN.md §4: algorithmic bytes of the whole pipeline = 248 B / camera sample + 352 B / expanded vertex + 12 B / pixel."""
    return 248 * stats_sum["camera_samples"] + 352 * stats_sum["vertices"] + 12 * pixels * steps


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, img):
    """--dump-outputs: what the timed path handed back in its last step, for comparing two builds output for output.  The frame whole when it fits in
    DUMP_LIMIT_BYTES, else the same seeded choice of pixels every run (their flat indices ride along, as float64: exact below 2^53)."""
    os.makedirs(out_dir, exist_ok=True)
    img = np.ascontiguousarray(img, dtype=np.float32)
    if img.nbytes <= DUMP_LIMIT_BYTES:
        np.save(os.path.join(out_dir, "image.npy"), img)
        return
    pixels = img.reshape(-1, img.shape[-1])
    n = (DUMP_LIMIT_BYTES - 4096) // (pixels.shape[1] * 4 + 8)        # (4 KB left for the two .npy headers)
    idx = np.sort(np.random.default_rng(0).choice(pixels.shape[0], size=n, replace=False))
    np.save(os.path.join(out_dir, "image_sample.npy"), pixels[idx])
    np.save(os.path.join(out_dir, "image_sample_index.npy"), idx.astype(np.float64))


def main():
    args = parse_args()
    run = extras(args)          # what this run does besides its headline (only with --full)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        _respawn_under_launcher(args)

    import torch
    import torch.distributed as dist

    from rustlight_amd import api, provenance, scenes
    from rustlight_amd import distributed as rd

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU fallback path exists)")
    n_dev = torch.cuda.device_count()
    env_world = int(os.environ.get("WORLD_SIZE", "1"))
    env_rank = int(os.environ.get("RANK", "0"))
    env_local = int(os.environ.get("LOCAL_RANK", "0"))
    # fewer devices than ranks (or RL_BENCH_SHARE_DEVICE=1): ranks share devices, RCCL cannot (one rank per device), so the reduce goes through gloo
    shared = env_world > n_dev or bool(os.environ.get("RL_BENCH_SHARE_DEVICE"))
    backend = os.environ.get("RL_BENCH_BACKEND") or ("gloo" if shared else "nccl")
    # the device is chosen BEFORE the process group exists and handed to it (device_id): RCCL then binds its communicator to this GPU at init,
    # not lazily to whatever device happens to be current at the first collective
    device_index = env_local % n_dev
    torch.cuda.set_device(device_index)
    dev = torch.device("cuda", device_index)
    who = {"rank": env_rank, "local_rank": env_local, "world": env_world, "device": device_index, "devices_visible": n_dev, "backend": backend,
           "master": f"{os.environ.get('MASTER_ADDR')}:{os.environ.get('MASTER_PORT')}", "HSA_ENABLE_IPC_MODE_LEGACY": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY"),
           "HIP_VISIBLE_DEVICES": os.environ.get("HIP_VISIBLE_DEVICES"), "ROCR_VISIBLE_DEVICES": os.environ.get("ROCR_VISIBLE_DEVICES"), "pid": os.getpid()}
    with _Watchdog("torch.distributed init + first collective", args.init_timeout, who):
        try:
            rank, world, local_rank = rd.init_from_env(args.gpus, backend, device=dev if backend == "nccl" else None, timeout_s=args.init_timeout)
            if world > 1:
                rd.max_over_ranks(1.0)          # first contact between the ranks (communicator setup over xGMI), outside every timed region
        except Exception as e:      # noqa: BLE001 — whatever RCCL / the store raises: say where, then fail
            print(f"bench.py: process-group init failed: {e!r}: {json.dumps(who)}", file=sys.stderr, flush=True)
            raise
    if world != args.gpus:
        raise SystemExit(f"bench.py --gpus {args.gpus} is running with WORLD_SIZE={world}: launch it with --nproc-per-node {args.gpus} (or without a launcher)")
    if world > 1:
        assert dist.is_initialized() and dist.get_world_size() == args.gpus, (dist.get_world_size(), args.gpus)
    # ---- N > 1 on a box that HAS N devices: the collective must be RCCL over N distinct GPUs, or the run is not a scaling measurement and must not look like one
    # (non-zero exit: the driver's SCALE record then shows the failure instead of a number measured through gloo or on shared devices)
    rccl_check = None
    if world > 1 and not shared:
        problems = []
        if backend != "nccl": problems.append(f"backend is {backend!r}, not nccl (= RCCL)")
        if n_dev < world: problems.append(f"{n_dev} devices visible for {world} ranks")
        try:
            props = torch.cuda.get_device_properties(device_index)
            ident = f"{getattr(props, 'uuid', '')}|{getattr(props, 'pci_bus_id', '')}|{getattr(props, 'pci_device_id', '')}|{device_index}"
        except Exception as e:      # noqa: BLE001
            ident = f"?{e!r}|{device_index}"
        with _Watchdog("the RCCL check (all_gather_object + all_reduce of ones)", args.init_timeout, who):
            idents = rd.gather_objects(ident)            # every rank's device identity, on every rank
            ones = torch.ones(1, device=dev)
            dist.all_reduce(ones)                        # a device-side collective: N ranks must have contributed
            torch.cuda.synchronize()
            if int(ones.item()) != world: problems.append(f"all_reduce of ones gave {ones.item()} on {world} ranks")
            if len(set(idents)) != world: problems.append(f"ranks do not sit on {world} distinct devices: {idents}")
            bad = rd.max_over_ranks(1.0 if problems else 0.0)
        rccl_check = {"backend": backend, "world_size": world, "devices_visible": n_dev, "distinct_devices": len(set(idents)), "all_reduce_of_ones": int(ones.item()), "ok": not problems}
        if bad:
            print(f"bench.py: --gpus {args.gpus} is not an RCCL run over {world} GPUs: {problems or 'another rank failed its check'}: {json.dumps(who)}", file=sys.stderr, flush=True)
            rd.finalize()
            raise SystemExit(4)

    # ONE explicit stream for everything a step enqueues (render, reduce, download): torch's default stream has handle 0, which the C-ABI
    # reads as "use the context's own stream" — the next step's framebuffer memset would then race the previous step's reduce / download
    work_stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(work_stream)
    stream = work_stream.cuda_stream
    assert stream != 0
    pipeline = {"auto": 0, "wavefront": 1, "fused": 2}[args.pipeline]
    STAT_KEYS = ("camera_samples", "vertices", "extension_rays", "shadow_rays", "iterations", "n_extend_launches", "kernel_launches")
    MS_KEYS = ("ms_raygen", "ms_extend", "ms_shade", "ms_shadow", "ms_other", "ms_prepass", "ms_eval_span")

    def build_scene(name, width, height, tris=0):
        if name == "cbox":
            return scenes.cbox(width, height), f"cbox {width}x{height} diffuse path"
        if name == "cbox_medium":
            return scenes.cbox_medium(width, height, 0.5), f"cbox + homogeneous medium sigma_s=0.5 {width}x{height}"
        tess = 32
        while 256 * 2 * tess * (tess - 1) + 14 < tris: tess += 1
        sd = scenes.living_room(width, height, tess=tess)
        return sd, f"living-room-class synthetic stand-in ({sd.n_triangles} tris, 6 BSDF types; the real pbrt-v3 living-room is not available) {width}x{height}"

    def time_workload(ctx, width, height, spp_total, stream_mode, numerics, steps, warmup, shard=(0, 1), pool=0, pipe=0, per_step=False):
        """`steps` timed renders (+ reduce + download) between barriers; returns the record the JSON lines are made of.  per_step (the `also` records of the slow default-mode
        configs only, never the headline): the device is synchronised after every step and each step's wall time kept, so that the record can quote its worst step."""
        fb = torch.zeros((height, width, 3), dtype=torch.float32, device=dev)
        host_fb = torch.zeros((height, width, 3), dtype=torch.float32).pin_memory() if rank == 0 else None

        def params(shard_index, shard_count):
            return api.path_params(spp=spp_total, shard_index=shard_index, shard_count=shard_count, pool_slots=pool, pipeline=pipe,
                                   stream_mode=api.STREAM_PER_SAMPLE if stream_mode == "per_sample" else api.STREAM_REFERENCE_ORDER,
                                   numerics={"exact": 0, "fast": 1}[numerics])

        reduce_events = []

        def step(seed):
            seeds = api.IndependentSampler(seed).block_seeds(width, height)              # same master stream on every rank
            _, st = ctx.render(seeds, params(*shard), out_device_ptr=fb.data_ptr(), stream=stream)
            if shard[1] > 1:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(work_stream)
                rd.reduce_framebuffer(fb)                                                 # one RCCL reduce over xGMI
                e1.record(work_stream)
                reduce_events.append((e0, e1))
            if rank == 0:
                host_fb.copy_(fb, non_blocking=True)                                      # framebuffer download (inside the timed region, §8(d))
            return st

        for w in range(warmup):
            step(1000 + w)
        rd.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step_ms = []
        if per_step:
            stats = []
            for s in range(steps):
                ts = time.perf_counter()
                stats.append(step(s))
                torch.cuda.synchronize()
                step_ms.append((time.perf_counter() - ts) * 1e3)
        else:
            stats = [step(s) for s in range(steps)]
        rd.barrier()
        torch.cuda.synchronize()
        dt = rd.max_over_ranks(time.perf_counter() - t0)
        agg = {k: sum(s[k] for s in stats) for k in STAT_KEYS}
        ms = {k: sum(s[k] for s in stats) for k in MS_KEYS}
        host_img = host_fb.numpy().copy() if rank == 0 else None
        # (this rank's wait for the slowest shard is part of its reduce time: the collective cannot start before every rank has arrived)
        reduce_ms = sum(a.elapsed_time(b) for a, b in reduce_events[-steps:]) / steps if reduce_events else 0.0
        return {"reduce_ms": reduce_ms, "dt": dt, "agg": agg, "ms": ms, "host_img": host_img, "params": params, "steps": steps, "samples_per_step": width * height * spp_total,
                "last_seed": steps - 1, "spp": spp_total, "stream_mode": stream_mode, "step_ms": step_ms,
                "overlapped": bool(stats[-1].get("overlapped")), "chunks": int(stats[-1].get("chunks", 0)),
                "spec": {k: stats[-1][k] for k in ("spec_group", "spec_samples", "spec_serial_samples", "spec_probe_samples")}}

    # ---- the headline workload
    sd, what = build_scene(args.scene, args.width, args.height, args.tris)
    spp_total = args.spp * world if args.scaling == "weak" else args.spp
    workload = {"cbox": f"{what} x{args.spp}spp-per-GPU (BASELINE configs[1]; configs[3] at 8 GPUs)" if args.scaling == "weak" else f"{what} x{args.spp}spp in total (BASELINE configs[1], strong scaling)",
                "cbox_medium": f"{what} x{args.spp}spp (BASELINE configs[4])", "living_room": f"{what} x{args.spp}spp (BASELINE configs[2])"}[args.scene]
    scene = api.Scene(sd)
    ctx = api.Context(scene, device_index)          # BVH build + upload: untimed, like the reference (mod.rs:280)
    main_rec = time_workload(ctx, args.width, args.height, spp_total, args.stream_mode, args.numerics, args.steps, args.warmup,
                             shard=(rank, world), pool=args.pool, pipe=pipeline)
    dt, agg, ms, host_img = main_rec["dt"], main_rec["agg"], main_rec["ms"], main_rec["host_img"]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, host_img)
    value = main_rec["samples_per_step"] * args.steps / dt / 1e6
    agg_all = rd.sum_over_ranks(agg)
    ranks = rd.gather_objects({"rank": rank, "device": device_index, "name": torch.cuda.get_device_name(device_index), "pid": os.getpid(),
                               "kernel_ms_per_step": ((ms["ms_other"] + ms["ms_prepass"]) or sum(ms.values())) / max(1, args.steps),
                               "reduce_ms_per_step": main_rec["reduce_ms"]})
    # ---- N > 1, --full: the same shards once more in rustlight's own reference-order streams (the drop-in default), so that one multi-GPU run answers for both
    # stream modes: per rank the chain pass (k_stream_spec), the evaluation pass (k_path_fused) and the reduce
    ref_multi = None
    if run["reference_order"]:
        rrec = time_workload(ctx, args.width, args.height, spp_total, "reference", "exact", 2, 1, shard=(rank, world))
        per_rank = rd.gather_objects({"rank": rank, "chain_ms": rrec["ms"]["ms_prepass"] / 2, "eval_span_ms": rrec["ms"]["ms_eval_span"] / 2, "eval_tail_after_chain_ms": rrec["ms"]["ms_other"] / 2,
                                      "overlapped": rrec["overlapped"], "reduce_ms": rrec["reduce_ms"], "chain_pass": rrec["spec"]})
        # the same shards with three frames in flight per rank (three contexts, one host thread each: the chain pass of a shard leaves most of its GPU idle — one wave per
        # block — and another frame's fills it); the frames' reduces follow in frame order on the main thread once every render has returned, so every rank issues the
        # same collectives in the same order.  A failure here is reported in the record, never raised: the headline above does not depend on it.
        import threading
        K_IF, F_IF = 3, 6
        in_flight = {"in_flight": K_IF, "frames": F_IF, "errors": None}
        errs = []
        ctxs, fbs, host_if = [ctx], [], None
        pp_if = api.path_params(spp=spp_total, shard_index=rank, shard_count=world, stream_mode=api.STREAM_REFERENCE_ORDER)

        def flight(c, frames):
            try:
                for f in frames:
                    ctxs[c].render(api.IndependentSampler(f if f >= 0 else 1000 + c).block_seeds(args.width, args.height), pp_if, out_device_ptr=fbs[max(f, 0)].data_ptr())
            except Exception as e:      # noqa: BLE001
                errs.append(repr(e))
        try:        # everything that can fail on ONE rank (memory) happens before the ranks agree to go on: no rank is left alone in a collective
            ctxs += [api.Context(scene, device_index) for _ in range(K_IF - 1)]
            fbs = [torch.zeros((args.height, args.width, 3), dtype=torch.float32, device=dev) for _ in range(F_IF)]
            host_if = torch.zeros((args.height, args.width, 3), dtype=torch.float32).pin_memory() if rank == 0 else None
            for c in range(1, K_IF):
                flight(c, [-1])             # warm-up of the new contexts (the first one rendered above)
        except Exception as e:      # noqa: BLE001
            errs.append(repr(e))
        if rd.max_over_ranks(1.0 if errs else 0.0) == 0.0:
            rd.barrier()
            torch.cuda.synchronize()
            t_if = time.perf_counter()
            th = [threading.Thread(target=flight, args=(c, list(range(c, F_IF, K_IF)))) for c in range(K_IF)]
            for t in th: t.start()
            for t in th: t.join()
            for f in range(F_IF):           # (every rank issues these whatever its threads reported)
                rd.reduce_framebuffer(fbs[f])
                if rank == 0:
                    host_if.copy_(fbs[f], non_blocking=True)
            rd.barrier()
            torch.cuda.synchronize()
            t_if = rd.max_over_ranks(time.perf_counter() - t_if)
            in_flight.update({"ms_per_step": t_if / F_IF * 1e3, "value": args.width * args.height * spp_total * F_IF / t_if / 1e6, "unit": "Msamples/s",
                              "image_crc32_last_frame": f"{zlib.crc32(host_if.numpy().tobytes()):08x}" if rank == 0 else None})
        else:
            in_flight["skipped"] = "a rank could not set its contexts up"
        for c in ctxs[1:]:
            c.close()
        in_flight["errors"] = errs or None
        if rank == 0:
            ref_multi = {"workload": f"cbox {args.width}x{args.height}x{spp_total}spp in RL_STREAM_REFERENCE_ORDER on {world} shards", "steps": 2, "ms_per_step": rrec["dt"] / 2 * 1e3,
                         "value": rrec["samples_per_step"] * 2 / rrec["dt"] / 1e6, "unit": "Msamples/s", "ranks": per_rank,
                         "image_crc32": f"{zlib.crc32(rrec['host_img'].tobytes()):08x}", "three_frames_in_flight": in_flight}

    # ---- N > 1, weak default, --full: the strong-scaling pair in the same invocation — the same frame as the 1-GPU run (spp in TOTAL, tiles split N ways), both
    # stream modes, 3 steps each: the N-GPU images must carry the CRCs the oracle gave for the 1-GPU frames (seed 2)
    strong = None
    if run["strong_scaling"]:
        strong = []
        for mode in ("per_sample", "reference"):
            srec = time_workload(ctx, args.width, args.height, args.spp, mode, "exact", 3, 1, shard=(rank, world))
            # (reference mode: the evaluation pass runs beside the chain pass — eval_span_ms is its own span, kernel_ms the critical path = chain pass + the tail left after it)
            per_rank = rd.gather_objects({"rank": rank, "kernel_ms": (srec["ms"]["ms_other"] + srec["ms"]["ms_prepass"]) / 3, "chain_ms": srec["ms"]["ms_prepass"] / 3,
                                          "eval_span_ms": srec["ms"]["ms_eval_span"] / 3, "reduce_ms": srec["reduce_ms"]})
            if rank == 0:
                crc_s = f"{zlib.crc32(srec['host_img'].tobytes()):08x}"
                want_s = oracle_crc("cbox", args.width, args.height, args.spp, mode, 2)
                strong.append({"workload": f"cbox {args.width}x{args.height}x{args.spp}spp in total on {world} shards, {mode} streams (strong scaling)", "stream_mode": mode, "steps": 3,
                               "ms_per_step": srec["dt"] / 3 * 1e3, "value": srec["samples_per_step"] * 3 / srec["dt"] / 1e6, "unit": "Msamples/s", "ranks": per_rank,
                               "image_crc32": crc_s, "oracle_crc32": want_s, "oracle_crc_match": None if want_s is None else want_s == crc_s})

    if rank == 0:
        # ---- --full: the N-GPU image must be the 1-GPU image, bit for bit (sums with zeros are exact): re-render the last step's
        # frame on this GPU alone, untimed, and compare CRCs
        crc = zlib.crc32(host_img.tobytes())
        crc_single = None
        if run["verify"]:
            seeds = api.IndependentSampler(args.steps - 1).block_seeds(args.width, args.height)
            single, _ = ctx.render(seeds, main_rec["params"](0, 1))
            crc_single = zlib.crc32(single.tobytes())
            if crc_single != crc:       # reported in the JSON (crc_match: false) rather than raised: the other ranks are waiting in a barrier
                print(f"ERROR: {world}-GPU image CRC {crc:08x} != 1-GPU image CRC {crc_single:08x}", file=sys.stderr)
        # ---- roofline.  Algorithmic bytes per unit:
        #   k_raygen 108 B/camera sample, k_extend 44 B/ray, k_shade 280 B/vertex, k_shadow 72 B/shadow ray,
        #   k_path_fused (all four stages in one persistent launch): the whole-pipeline figure
        #   248 B/camera sample + 352 B/expanded vertex + 12 B/pixel; k_stream_chain (first pass of reference-order streams): 32 B of sampler
        #   state written per camera sample + 44 B per extension ray
        pix = args.width * args.height / world
        pipe_bytes = pipeline_bytes(agg, pix, args.steps)
        fused = ms["ms_other"] > 0.0
        names = {"ms_raygen": "k_raygen", "ms_extend": "k_extend", "ms_shade": "k_shade", "ms_shadow": "k_shadow", "ms_other": "k_path_fused"}
        per_unit = {"ms_raygen": 108, "ms_extend": 44, "ms_shade": 280, "ms_shadow": 72}
        units = {"ms_raygen": agg["camera_samples"], "ms_extend": agg["extension_rays"], "ms_shade": agg["extension_rays"], "ms_shadow": agg["shadow_rays"]}
        n_launch = {k: max(1, agg["n_extend_launches"]) for k in per_unit}
        kernels = {}
        for k in per_unit:
            if ms[k] > 0:
                avg = ms[k] / n_launch[k]
                gbs = per_unit[k] * units[k] / n_launch[k] / (avg * 1e-3) / 1e9
                kernels[names[k]] = {"avg_launch_ms": avg, "launches": n_launch[k], "algorithmic_bytes_per_unit": per_unit[k], "achieved_GBps": gbs, "frac": gbs / PEAK_HBM_GBPS}
        if fused:
            # two passes (reference-order streams): the evaluation kernel runs BESIDE the chain pass, `ms_other` is only what of it was left after the chain pass had
            # ended — its roofline divides by its own span, first launch to last completion (rl_render_stats.ms_eval_span; ADVICE r5: dividing the pipeline's
            # bytes by the tail inflated the fraction past 1)
            two_pass_run = ms["ms_prepass"] > 0.0
            avg = (ms["ms_eval_span"] if two_pass_run and ms["ms_eval_span"] > 0.0 else ms["ms_other"]) / args.steps
            gbs = pipe_bytes / args.steps / (avg * 1e-3) / 1e9
            kernels["k_path_fused"] = {"avg_launch_ms": avg, "launches": args.steps, "algorithmic_bytes_per_unit": "248/sample + 352/vertex + 12/pixel",
                                       "achieved_GBps": gbs, "frac": gbs / PEAK_HBM_GBPS}
            if two_pass_run:
                kernels["k_path_fused"].update({"overlapped_with_chain_pass": main_rec["overlapped"], "tail_after_chain_pass_ms": ms["ms_other"] / args.steps,
                                                "note": "avg_launch_ms = the evaluation pass's span (its launches run on several streams beside the chain kernel, sharing the chip with it)"})
        if ms["ms_prepass"] > 0.0:
            avg = ms["ms_prepass"] / args.steps
            gbs = (32 * agg["camera_samples"] + 44 * agg["extension_rays"]) / args.steps / (avg * 1e-3) / 1e9
            kernels["k_stream_spec" if main_rec["spec"]["spec_group"] else "k_stream_chain"] = {"avg_launch_ms": avg, "launches": args.steps, "algorithmic_bytes_per_unit": "32/sample + 44/extension ray",
                                         "achieved_GBps": gbs, "frac": gbs / PEAK_HBM_GBPS}
        dominant = max(kernels, key=lambda k: kernels[k]["avg_launch_ms"] * kernels[k]["launches"])
        # PMC numbers are NOT collected in this run (rocprofv3 --pmc needs its own passes: scratch/pmc_collect.sh).  They are quoted
        # only when they were collected on this very kernel source (hash of csrc/kernels + flags), with their provenance.
        src_hash = provenance.kernel_source_hash()
        traffic, pmc_entry, live = None, None, None
        try:
            live = json.load(open(os.path.join(ROOT, "profiles", "pmc_live.json")))
            key = f"{args.scene}{':tris' + str(args.tris) if args.tris else ''}:{args.width}x{args.height}x{args.spp}:{args.stream_mode}:{args.numerics}"
            e = live.get(key)
            if e and e.get("kernel") == dominant and world == 1:
                pmc_entry = dict(e, current=(e.get("kernel_src_hash") == src_hash))
                if pmc_entry["current"]:
                    traffic = e.get("hbm_bytes_per_launch")
        except Exception:
            pass
        roofline = {"bound": (pmc_entry or {}).get("bound", "valu"), "kernel": dominant,
                    "achieved": kernels[dominant]["achieved_GBps"], "peak": PEAK_HBM_GBPS, "unit": "GB/s", "frac": kernels[dominant]["frac"],
                    "note": "achieved = ALGORITHMIC bytes (SURVEY §8(d): state a wavefront pipeline would stream) / kernel time; the fused kernel keeps that state in "
                            "registers / LDS, so measured HBM traffic (`traffic`) is far below it and the kernel is bound by VALU issue + latency, not by HBM",
                    "traffic": traffic, "avg_launch_ms": kernels[dominant]["avg_launch_ms"],
                    "launches": kernels[dominant]["launches"], "kernels": kernels,
                    "pipeline_algorithmic_GBps": pipe_bytes / dt / 1e9, "pipeline_frac": pipe_bytes / dt / 1e9 / PEAK_HBM_GBPS,
                    "rays_per_s": (agg_all["extension_rays"] + agg_all["shadow_rays"]) / dt,
                    "kernel_src_hash": src_hash, "pmc": pmc_entry}
        # the honest utilisation, first-class next to the nominal `frac`: what share of the VALU issue slots is busy, how many of the 64 lanes of an issued instruction are
        # live, and the product (None when this workload has no counter summary; `pmc_current` false when it was collected on other kernel sources)
        util = utilisation_fields(live, f"{args.scene}{':tris' + str(args.tris) if args.tris else ''}:{args.width}x{args.height}x{args.spp}:{args.stream_mode}:{args.numerics}", dominant, src_hash) if world == 1 else None
        roofline.update({k: (util or {}).get(k) for k in ("valu_issue_busy", "lane_utilisation", "valu_lane_slots_used", "wave_time_waiting", "pmc_current")})

        # ---- `also`: the other BASELINE configurations and stream modes, timed the same way in this process (--full, default single-GPU run only)
        also, reference_order_value = None, None
        if run["also"]:
            also = []

            def sub(tag, rec, what, extra=None, scene_name="cbox"):
                a, m = rec["agg"], rec["ms"]
                width, height = rec["host_img"].shape[1], rec["host_img"].shape[0]
                chain_kernel = "k_stream_spec" if rec["spec"]["spec_group"] else "k_stream_chain"
                two_pass_rec = m["ms_prepass"] > 0
                # two passes: k_path_fused's entry is its own span (it runs beside the chain pass), the step's critical path is chain pass + the tail left after it
                kernel_ms = {k: v / rec["steps"] for k, v in (("k_path_fused", m["ms_eval_span"] if two_pass_rec and m["ms_eval_span"] > 0 else m["ms_other"]), (chain_kernel, m["ms_prepass"])) if v > 0}
                kms = (m["ms_prepass"] + m["ms_other"]) / rec["steps"] if two_pass_rec else sum(kernel_ms.values())
                r = {"workload": tag, "what": what, "steps": rec["steps"], "ms_per_step": rec["dt"] / rec["steps"] * 1e3,
                     "value": rec["samples_per_step"] * rec["steps"] / rec["dt"] / 1e6, "unit": "Msamples/s",
                     "kernel_ms": {k: round(v, 3) for k, v in kernel_ms.items()}, "kernel_ms_total": round(kms, 3),
                     "mean_vertices_per_sample": a["vertices"] / max(1, a["camera_samples"]),
                     "rays_per_s": (a["extension_rays"] + a["shadow_rays"]) / rec["dt"],
                     "frac": pipeline_bytes(a, width * height, rec["steps"]) / rec["steps"] / (kms * 1e-3) / 1e9 / PEAK_HBM_GBPS if kms else None,
                     "image_crc32": f"{zlib.crc32(rec['host_img'].tobytes()):08x}", "image_mean": float(rec["host_img"].mean())}
                want = oracle_crc(scene_name, width, height, rec["spp"], rec["stream_mode"], rec["last_seed"])
                r["oracle_crc32"] = want
                r["oracle_crc_match"] = None if want is None else want == r["image_crc32"]        # the last timed frame against the CPU oracle's render of it
                if rec["spec"]["spec_group"]:
                    r["chain_pass"] = dict(rec["spec"], note="k_stream_spec: lanes per block, samples walked speculatively / serially / by the estimate probes in the last step")
                if m["ms_prepass"] > 0:
                    r["overlapped"], r["chunks"] = rec["overlapped"], rec["chunks"]
                    r["eval_tail_after_chain_ms"] = round(m["ms_other"] / rec["steps"], 3)
                    r["overlap_note"] = ("reference-order streams: k_path_fused runs BESIDE the chain pass on the context's low-priority streams, over lists of complete blocks "
                                         "(DESIGN.md 4 (4)); kernel_ms.k_path_fused is its own span (first launch to last completion), eval_tail_after_chain_ms the part of it "
                                         "left after the chain pass had ended, kernel_ms_total = chain pass + that tail = the step's critical path")
                if rec["step_ms"]:
                    sm = sorted(rec["step_ms"])
                    per = [rec["samples_per_step"] / (t * 1e-3) / 1e6 for t in sm]          # fastest step first
                    r["step_ms"] = [round(t, 1) for t in rec["step_ms"]]
                    r["value_min"], r["value_median"], r["value_max"] = per[-1], per[len(per) // 2], per[0]
                    r["value_note"] = "`value` = all timed steps together; value_min = the WORST single step (each step synchronised and timed on its own)"
                # utilisation of the record's longest kernel, when profiles/pmc_live.json holds its counters
                longest = max(kernel_ms, key=kernel_ms.get) if kernel_ms else None
                u = utilisation_fields(live, f"{scene_name}:{width}x{height}x{rec['spp']}:{rec['stream_mode']}:exact", longest, src_hash)
                if u is not None:
                    r["utilisation"] = dict(u, kernel=longest)
                r.update(extra or {})
                also.append(r)
                return r

            r = time_workload(ctx, 1920, 1080, 128, "reference", "exact", 3, 1, per_step=True)
            rr = sub("cbox_1080p_128spp_reference_order", r, "BASELINE configs[1] in RL_STREAM_REFERENCE_ORDER: rustlight's own stream assignment (one sampler per 16x16 block, "
                     "src/integrators/mod.rs:420-435), the plugin / CLI default; two passes: k_stream_spec (the block chains, speculative windows) + k_path_fused")
            reference_order_value = rr["value"]
            # ---- the same frames with three of them in flight: three contexts of the scene, one host thread each (a frame's render is a chain of dependent launches whose
            # tail leaves most of the chip idle; another context's frame fills it).  Timed like a step loop: barrier + synchronize, the frames dealt round-robin to the
            # contexts, each rendered into its own pinned host buffer (rl_render_path + download), join + synchronize.  Same frames, same images as one after the other.
            import threading
            K_IN_FLIGHT = 3
            ctxs = [ctx]
            try:
                ctxs += [api.Context(scene, device_index) for _ in range(K_IN_FLIGHT - 1)]
            except Exception:       # noqa: BLE001 — in_flight_record then fails on the missing context and is reported below
                pass

            def in_flight_record(tag, what, stream_mode, n_frames, oracle):
                bufs = [torch.zeros((1080, 1920, 3), dtype=torch.float32).pin_memory() for _ in range(3)]       # frames 0, 1, 2 are kept (frame 2 is the one the oracle's table holds), later ones land on frame 0's buffer
                pp_if = api.path_params(spp=128, stream_mode=stream_mode)
                seeds_f = [api.IndependentSampler(f).block_seeds(1920, 1080) for f in range(n_frames)]
                scratch = [torch.zeros((1080, 1920, 3), dtype=torch.float32).pin_memory() for _ in range(K_IN_FLIGHT)]
                errs = []

                def flight(c, frames):
                    try:
                        for f in frames:
                            dst = bufs[f] if 0 <= f < 3 else scratch[c]
                            ctxs[c].render(seeds_f[f] if f >= 0 else api.IndependentSampler(1000 + c).block_seeds(1920, 1080), pp_if, out_host_ptr=dst.data_ptr())
                    except Exception as e:      # noqa: BLE001
                        errs.append(repr(e))
                for c in range(K_IN_FLIGHT):
                    flight(c, [-1])             # warm-up: every context renders one frame alone (its buffers get allocated)
                torch.cuda.synchronize()
                t_if = time.perf_counter()
                th = [threading.Thread(target=flight, args=(c, list(range(c, n_frames, K_IN_FLIGHT)))) for c in range(K_IN_FLIGHT)]
                for t in th: t.start()
                for t in th: t.join()
                torch.cuda.synchronize()
                t_if = time.perf_counter() - t_if
                crc_if = f"{zlib.crc32(bufs[2].numpy().tobytes()):08x}"
                rec = {"workload": tag, "what": what, "frames": n_frames, "in_flight": K_IN_FLIGHT, "ms_per_step": t_if / n_frames * 1e3, "value": 1920 * 1080 * 128 * n_frames / t_if / 1e6, "unit": "Msamples/s",
                       "image_crc32_frame_2": crc_if, "oracle_crc32": oracle, "oracle_crc_match": None if oracle is None else oracle == crc_if, "errors": errs or None}
                also.append(rec)
                return rec
            reference_order_in_flight = {"value": None}
            try:        # (an extra: a failure here — memory — must not cost the line the driver reads)
                reference_order_in_flight = in_flight_record(
                    "cbox_1080p_128spp_reference_order_3_in_flight", "the reference-order frames above, three in flight (three device contexts, one host thread each; rustlight_amd.api.render_in_flight / "
                    "IntegratorPathTracing.frames_in_flight, `rustlight-amd --frames-in-flight 3 -a ...`): throughput of independent frames, not the latency of one", api.STREAM_REFERENCE_ORDER, 12, rr["oracle_crc32"])
                in_flight_record("cbox_1080p_128spp_3_in_flight", "the headline's frames (per-sample streams), three in flight: the same", api.STREAM_PER_SAMPLE, 18,
                                 oracle_crc("cbox", 1920, 1080, 128, "per_sample", 2))
            except Exception as e:      # noqa: BLE001
                also.append({"workload": "frames_in_flight", "error": repr(e)})
            for c in ctxs[1:]:
                try: c.close()
                except Exception: pass      # noqa: BLE001
            ctx.close()
            for tag, name, w, h, steps, what in (
                    ("cbox_1080x1080_128spp", "cbox", 1080, 1080, 3, "BASELINE configs[1] on a square frame (no pixels looking past the box: V/sample 2.1 instead of 1.15)"),
                    ("cbox_medium_1080p_128spp", "cbox_medium", 1920, 1080, 3, "BASELINE configs[4]: cbox + homogeneous medium sigma_s = 0.5"),
                    ("living_room_standin_1080p_128spp", "living_room", 1920, 1080, 3, "BASELINE configs[2] stand-in: 508 k triangles, 6 BSDF types, BVH streamed from L2 / Infinity Cache")):
                sd2, _ = build_scene(name, w, h)
                t_build = time.perf_counter()
                ctx2 = api.Context(api.Scene(sd2), device_index)
                t_build = time.perf_counter() - t_build
                r = time_workload(ctx2, w, h, 128, "per_sample", "exact", steps, 1)
                sub(tag, r, what, {"context_build_s": round(t_build, 2), "triangles": int(sd2.n_triangles)}, scene_name=name)
                if name != "cbox":
                    # the drop-in default on the two slow configs: rustlight's own reference-order streams, THREE timed steps after one
                    # warm-up render, each synchronised and timed on its own (value_min = the worst of them), the last frame (seed 2) against the oracle's CRC —
                    # the weakest numbers of the product's default mode, driver-timed
                    r = time_workload(ctx2, w, h, 128, "reference", "exact", 3, 1, per_step=True)
                    sub(tag + "_reference_order", r, what + " — in RL_STREAM_REFERENCE_ORDER (the plugin / CLI default): chain pass + k_path_fused", {"triangles": int(sd2.n_triangles)}, scene_name=name)
                ctx2.close()

        cpu = None
        if run["cpu_baseline"]:
            from oracle import orc
            orc.use_timing_build()        # -O3 / libm / FMA build of the same restatement; never the checker
            cw, ch, cspp = args.width, args.height, max(1, args.spp // 4)   # bounded sample of the same workload: same scene and resolution, 1/4 of the spp (~10 s of CPU work over three passes)
            osc = orc.Scene(scenes.cbox(cw, ch) if args.scene == "cbox" else (scenes.cbox_medium(cw, ch, 0.5) if args.scene == "cbox_medium" else sd))
            # cores this process may really use: the GPU boxes report 256 hardware threads but run under a cgroup CPU quota
            # (cpu.max = 16 CPUs); more runnable threads than quota only adds throttling
            ncpu = len(os.sched_getaffinity(0))
            try:
                quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
                if quota != "max":
                    ncpu = max(1, min(ncpu, int(-(-int(quota) // int(period)))))
            except (OSError, ValueError):
                pass
            osc.render(master_seed=1, spp=1, stream_mode=0, threads=ncpu)             # warm up / page in
            runs = []
            for _ in range(3):      # the host is shared and noisy: report the best of three passes (all three listed)
                t1 = time.perf_counter()
                _, ost = osc.render(master_seed=0, spp=cspp, stream_mode=0, threads=ncpu)
                runs.append(cw * ch * cspp / (time.perf_counter() - t1) / 1e6)
                if sum(cw * ch * cspp / r / 1e6 for r in runs) > 30.0:
                    break
            cpu = {"value": max(runs), "unit": "Msamples/s", "cores": ost["threads"], "kind": "port", "runs": [round(r, 2) for r in runs],
                   "sample": f"{args.scene} {cw}x{ch}x{cspp}spp, reference-order streams, CPU restatement of rustlight `path` (C++, -O3 timing build), {ost['threads']} threads = CPUs available to the process (affinity / cgroup quota; the host has {os.cpu_count()} hardware threads), best of {len(runs)}"}
        try:
            rccl = ".".join(str(x) for x in torch.cuda.nccl.version())
        except Exception:
            rccl = None
        out = {"metric": "Msamples/s (paths/s) at 1080p x 128spp cbox", "value": value, "unit": "Msamples/s", "n_gpus": world, "steps": args.steps,
               "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None, "full": args.full,
               "dtype": "f32", "data": "synthetic",
               "config": {"workload": workload, "spp_total": spp_total, "stream_mode": args.stream_mode, "numerics": args.numerics,
                          "pipeline": (f"two passes: {'k_stream_spec' if main_rec['spec']['spec_group'] else 'k_stream_chain'} + k_path_fused" if ms["ms_prepass"] > 0 else "fused (k_path_fused)") if fused else "wavefront (raygen/extend/shade/shadow)",
                          "parallelism": f"tile-shard x{world} + 1 RCCL reduce",
                          "timed_region": "rl_render_path + framebuffer reduce (N > 1) + framebuffer download to pinned host memory (SURVEY §8(d))",
                          "mean_vertices_per_sample": agg_all["vertices"] / max(1, agg_all["camera_samples"]),
                          "image_mean": float(host_img.mean())},
               "distributed": {"world_size": world, "backend": backend if world > 1 else None, "rccl_version": rccl, "devices_visible": n_dev, "devices_shared": bool(shared and world > 1),
                               "ranks": ranks, "image_crc32": f"{crc:08x}", "single_gpu_image_crc32": None if crc_single is None else f"{crc_single:08x}",
                               "crc_match": None if crc_single is None else crc_single == crc},
               "roofline": roofline, "cpu_baseline": cpu}
        # (N > 1: the reduced N-shard frame against the oracle's render of the WHOLE frame at spp_total — BASELINE configs[3] is `--gpus 8 --steps 1`: cbox 1080p x 1024 spp, seed 0)
        want = oracle_crc(args.scene, args.width, args.height, spp_total, args.stream_mode, args.steps - 1) if run["oracle_crc"] and args.numerics == "exact" and args.tris == 0 else None
        out["oracle_crc32"] = want
        out["oracle_crc_match"] = None if want is None else want == f"{crc:08x}"        # the last timed frame == the CPU oracle's render of the same frame (tests/golden/bench_crcs.json)
        out["distributed"]["rccl_check"] = rccl_check
        if strong is not None:
            out["strong_scaling"] = strong
        if ref_multi is not None:
            out["reference_order_value"] = ref_multi["value"]
            out["reference_order_in_flight_value"] = ref_multi["three_frames_in_flight"].get("value")
            out["reference_order"] = ref_multi
        if also is not None:
            out["reference_order_value"] = reference_order_value
            # the default mode's weakest step over ALL configs the line times in it (cfg 2, cfg 5, the cfg 3 stand-in; three steps each): what "every config >= X" may quote
            worst = [a_["value_min"] for a_ in also if a_.get("workload", "").endswith("reference_order") and a_.get("value_min") is not None]
            out["reference_order_worst_step_value"] = min(worst) if worst else None
            out["reference_order_oracle_crc_match"] = rr["oracle_crc_match"]
            out["reference_order_in_flight_value"] = reference_order_in_flight["value"]      # three independent frames in flight (see `also`); `reference_order_value` is one frame at a time
            out["also"] = also
        print(json.dumps(out))
        sys.stdout.flush()
    rd.barrier()
    rd.finalize()


if __name__ == "__main__":
    main()
