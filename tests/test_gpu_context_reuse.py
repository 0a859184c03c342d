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


# ---- generation under the `no_events` option: the three entry points time their kernels unless the context says not to, and the option changes nothing else
def _generate(ctx, case):
    sampler = api.IndependentSampler(3)
    if case == "plane":
        made, st = ctx.plane_generate(sampler, 64, "average")
    else:
        made, st = ctx.vpl_generate(sampler, nb_vpl=300, option_vpl=api.VPL_VOLUME, streams=case)
    return made.words(), made.info(), tuple(int(w) for w in sampler.s.s), st


@pytest.mark.parametrize("case", ["reference", "per_path", "plane"])
def test_generation_obeys_no_events(built, case):
    ctx = api.Context(api.Scene(scenes.cbox_medium(32, 24, 1.0)), 0)
    words, info, state, st = _generate(ctx, case)
    assert st["ms_prepass"] > 0, st
    with ctx.options(no_events=1):
        words_off, info_off, state_off, st_off = _generate(ctx, case)
    assert st_off["ms_prepass"] == 0.0, st_off
    np.testing.assert_array_equal(words_off, words)
    assert info_off == info and state_off == state
    assert state != tuple(int(w) for w in api.IndependentSampler(3).s.s)      # (the call did advance the sampler)
    ctx.close()
