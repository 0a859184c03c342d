"""One context, render kinds interleaved: every call's image and counters are those of the same call on a fresh context.  The context's scratch buffers
(tables, recorded sampler states, parking buffer, statistics rows, overflow stacks) are shared by every render kind and grown on demand; the light tracer's
splat image lives in the buffer of the recorded sampler states.  A buffer a call reuses must not carry anything over from the calls before it."""
import numpy as np
import pytest

from rustlight_amd import api, scenes

pytestmark = pytest.mark.gpu

W, H = 160, 200


def _comparable(st):
    # everything but the timings, and the launch count of an overlapped evaluation pass (its launches follow what the host's polls find complete)
    return {k: v for k, v in st.items() if not k.startswith("ms_") and k != "render_ms" and not (k == "kernel_launches" and st["overlapped"])}


def _render(ctx, kind, seed, options, kw):
    seeds = api.IndependentSampler(seed).block_seeds(W, H)
    with ctx.options(**options):
        if kind == "path":
            return ctx.render(seeds, api.path_params(**kw))
        return getattr(ctx, "render_" + kind)(seeds, **kw)


def test_interleaved_render_kinds_match_fresh_contexts(built):
    sd = scenes.cbox(W, H)
    scene = api.Scene(sd)
    shared = api.Context(scene, 0)
    calls = [
        ("path", 1, {}, dict(spp=8, stream_mode=api.STREAM_PER_SAMPLE, sample_split=4)),
        ("light", 2, {}, dict(spp=4)),
        ("path", 3, dict(state_budget_mb=1), dict(spp=24, stream_mode=api.STREAM_REFERENCE_ORDER)),
        ("direct", 4, {}, dict(spp=6, stream_mode=api.STREAM_REFERENCE_ORDER)),
        ("ao", 5, {}, dict(spp=4, stream_mode=api.STREAM_STRATIFIED)),
        ("light", 6, {}, dict(spp=3)),
        ("path", 7, {}, dict(spp=16, stream_mode=api.STREAM_PER_SAMPLE, sample_split=4)),     # buffers grow
        ("path", 8, {}, dict(spp=4, stream_mode=api.STREAM_PER_SAMPLE, sample_split=2)),      # ... and are reused
    ]
    for kind, seed, options, kw in calls:
        img, st = _render(shared, kind, seed, options, kw)
        fresh = api.Context(scene, 0)
        ref, rst = _render(fresh, kind, seed, options, kw)
        fresh.close()
        what = f"{kind} {options} {kw}"
        np.testing.assert_array_equal(img, ref, err_msg=what)
        assert _comparable(st) == _comparable(rst), what
        assert img.any() and st["camera_samples"] == kw["spp"] * W * H, what
        if options:
            assert st["chunks"] >= 2, (what, st["chunks"])
        if kind == "light":
            assert st["splats"] > 0, what
    shared.close()
