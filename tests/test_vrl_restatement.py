"""The virtual ray lights without a GPU: the numpy restatement (tests/vrl_restatement.py) against a literal per-sample transcription of the reference's text
(src/integrators/explicit/vol_primitives.rs:201-253, 711-764) — one sampler walked draw by draw, one scalar float32 operation at a time — on a few tiny cases,
and the edge rules of the roulette: avg == 0, a NaN or infinite radiance, zero radiance."""
import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import beam_restatement as R
from tests import bre_restatement as B
from tests import vrl_restatement as V
from tests.test_beam_restatement import _color_times, _dot, _scalar_gather

F32 = np.float32


def _color_over(c, s):
    """Color / f32 (structure.rs): a zero or non-finite divisor gives black."""
    return (c / s).astype(np.float32) if (np.isfinite(s) and s != 0) else np.zeros(3, np.float32)


def _contribute_vrl(sc, o, d, length, rad, medium, ro, rd, tnear, tfar, next_f32):
    """PhotonBeam::contribute_vrl (vol_primitives.rs:201-253), statement by statement: (Color, visible)."""
    with np.errstate(all="ignore"):
        t_cam = F32(F32(F32(tfar - tnear) * F32(next_f32())) + tnear)
        t_vrl = F32(length * F32(next_f32()))
        inv_pdf = F32(length * F32(tfar - tnear))
        p_vrl = (o + (d * t_vrl).astype(np.float32)).astype(np.float32)
        p_cam = (ro + (rd * t_cam).astype(np.float32)).astype(np.float32)
        if not sc.visible(p_cam[None, :], p_vrl[None, :])[0]:
            return np.zeros(3, np.float32), False
        d_cam_vrl = (p_vrl - p_cam).astype(np.float32)
        dist = F32(np.sqrt(_dot(d_cam_vrl, d_cam_vrl)))
        sigma_t = (np.asarray(medium.sigma_a, np.float32) + np.asarray(medium.sigma_s, np.float32)) * F32(1.0)
        transmittance_cam = B._expf(-_color_times(sigma_t, t_cam))
        transmittance_vrl = B._expf(-_color_times(sigma_t, dist))
        iso = F32(F32(1.0) / F32(F32(np.pi) * F32(4.0)))
        phase_func_vrl = np.asarray(medium.sigma_s, np.float32) * iso
        phase_func_cam = np.asarray(medium.sigma_s, np.float32) * iso
        contrib = ((((rad * phase_func_vrl) * phase_func_cam) * transmittance_cam) * transmittance_vrl).astype(np.float32)
        return _color_over(_color_times(contrib, inv_pdf), F32(dist * dist)), True


def _scalar_render(sc, sd, words, n_paths, seeds, spp, radius, seed_variant=0):
    """The camera loop of vol_primitives.rs:711-790 with the VRL arm, one sample after the other on the block's own sampler."""
    w = np.ascontiguousarray(words, np.uint32).reshape(-1, api.BEAM_WORDS)
    beams = [r for r in w if r[7] & 1]                                  # .partition(|b| b.from_surface)
    vrls = [r for r in w if not (r[7] & 1)]
    with np.errstate(all="ignore"):
        total = F32(0.0)
        for r in vrls:
            rad = r.view(np.float32)[8:11]
            total = F32(total + np.fmax(rad[0], np.fmax(rad[1], rad[2])))
        avg = F32(total / F32(len(vrls))) if vrls else F32(0.0)
    sub = R.split(np.asarray(beams, np.uint32))
    tree = R.build_tree(sub, radius)
    norm = F32(F32(1.0) / F32(n_paths))
    img = np.zeros((sd.height, sd.width, 3), np.float32)
    st = {"camera_samples": 0, "rng_draws": 0, "beams_accepted": 0, "vrl_accepted": 0, "vrl_visible": 0}
    nby = (sd.height + 15) // 16
    for b, seed in enumerate(np.asarray(seeds, np.uint64)):
        bx, by = (b // nby) * 16, (b % nby) * 16
        bw, bh = min(16, sd.width - bx), min(16, sd.height - by)
        rng = orc.Rng(int(seed), seed_variant)

        def next_f32():
            st["rng_draws"] += 1
            return rng.next_f32()

        for ix in range(bw):
            for iy in range(bh):
                acc = np.zeros(3, np.float32)
                for _ in range(spp):
                    u = F32(bx + ix) + F32(next_f32())
                    v = F32(by + iy) + F32(next_f32())
                    ro, rd = sc.camera_generate(float(u), float(v))
                    t, _, _, mesh, _ = sc.trace(ro[None, :], rd[None, :])
                    tfar = F32(t[0]) if mesh[0] >= 0 else R.F32_MAX
                    c, n = _scalar_gather(tree, sub, radius, sd.medium, norm, ro, rd, tfar)
                    st["beams_accepted"] += n
                    for r in vrls:
                        f = r.view(np.float32)
                        with np.errstate(all="ignore"):
                            cm = np.fmax(f[8], np.fmax(f[9], f[10]))
                            rr = np.fmin(F32(F32(cm / avg) * F32(0.01)), F32(1.0))
                        if rr >= F32(next_f32()):
                            st["vrl_accepted"] += 1
                            val, visible = _contribute_vrl(sc, f[0:3], f[4:7], f[3], f[8:11], sd.medium, ro, rd, R.TNEAR, tfar, next_f32)
                            st["vrl_visible"] += int(visible)
                            c = c + _color_times(_color_over(val, rr), norm)
                    acc = acc + c
                    st["camera_samples"] += 1
                img[by + iy, bx + ix] = acc * (F32(1.0) / F32(spp))
    return img, st


def _case(seed, n_vrl, bright_every, radiance=(40.0, 30.0, 20.0)):
    """Four surface beams and n_vrl VRLs, interleaved: every bright_every-th VRL bright (rr = 0.01 * bright_every, up to the dim ones' share), the next one dim
    (rr of some 1e-4), the rest black (rr = 0: one draw each)."""
    rs = np.random.RandomState(seed)

    def cloud(n, lo, hi, from_surface, rad):
        o = rs.uniform((-0.8, 0.2, -0.8), (0.8, 1.8, 0.8), (n, 3)).astype(np.float32)
        d = rs.normal(size=(n, 3))
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        return R.beam_words(o, rs.uniform(lo, hi, n).astype(np.float32), d, rad, from_surface=from_surface)

    rad = np.zeros((n_vrl, 3), np.float32)
    rad[::bright_every] = radiance
    rad[1::bright_every] = (0.01, 0.02, 0.005)                            # dim ones: a small rr
    surface = cloud(4, 0.4, 1.2, True, rs.uniform(0.5, 2.0, (4, 3)))
    vr = cloud(n_vrl, 0.0, 0.7, False, rad)
    words = np.concatenate([surface[:2], vr[: n_vrl // 2], surface[2:], vr[n_vrl // 2:]])      # the partition keeps both orders
    return words


@pytest.mark.parametrize("w,h,spp,seed,n_vrl,every,sd_kw", [(5, 3, 2, 1, 150, 75, {}), (9, 5, 1, 2, 200, 50, {"sigma_a": 0.3}), (3, 4, 3, 3, 120, 40, {"g": 0.5})])
def test_restatement_equals_the_scalar_transcription(built, w, h, spp, seed, n_vrl, every, sd_kw):
    sd = scenes.cbox_medium(w, h, 1.0, **sd_kw)
    sc = orc.Scene(sd)
    words = _case(seed, n_vrl, every)
    seeds = orc.block_seeds(seed, w, h)
    img, st, detail = V.render(sc, sd, words, 3, seeds, spp, 0.3)
    want, want_st = _scalar_render(sc, sd, words, 3, seeds, spp, 0.3)
    for k in want_st:
        assert st[k] == want_st[k], k
    np.testing.assert_array_equal(img.view(np.uint32), want.view(np.uint32))
    assert st["vrl_accepted"] >= st["vrl_visible"] > 0 and st["beams_accepted"] > 0, st
    assert np.abs(detail["c"] - detail["c_beams"]).max() > 0
    assert st["rng_draws"] == st["camera_samples"] * (2 + n_vrl) + 2 * st["vrl_accepted"]
    # the chained starts: pixel c of a block starts where the samples before it ended
    starts = detail["starts"][0]
    assert starts[0] == 0 and all(b > a for a, b in zip(starts, starts[1:]))


def test_three_shards_partition_the_walk(built):
    sd = scenes.cbox_medium(33, 17, 1.0)
    sc = orc.Scene(sd)
    words = _case(4, 10, 2)
    seeds = orc.block_seeds(4, 33, 17)
    whole = V.render(sc, sd, words, 2, seeds, 1, 0.3)
    parts = [V.render(sc, sd, words, 2, seeds, 1, 0.3, 0, k, 3) for k in range(3)]
    np.testing.assert_array_equal(parts[0][0] + parts[1][0] + parts[2][0], whole[0])
    for k in V.KEYS:
        assert sum(p[1][k] for p in parts) == whole[1][k], k


def _vrl(rad):
    rad = np.asarray(rad, np.float32).reshape(-1, 3)
    return R.beam_words(np.zeros((rad.shape[0], 3)), 1.0, [(1.0, 0.0, 0.0)], rad, from_surface=False)


def test_roulette_rules():
    # equal VRLs: (m / m) * 0.01
    avg, rr = V.roulette(_vrl([(2.0, 1.0, 0.5)] * 7))
    assert avg == F32(2.0) and (rr == F32(0.01)).all()
    # the sum runs in f32 in storing order
    rad = [(1e8, 0, 0)] + [(1.0, 0, 0)] * 9
    avg, _ = V.roulette(_vrl(rad))
    assert avg == F32(1e8) / F32(10.0)                                   # 1e8 + 1 == 1e8 in f32, nine times
    avg, _ = V.roulette(_vrl(rad[::-1]))
    assert avg == F32(F32(9.0) + F32(1e8)) / F32(10.0)
    # a hundredth of the mean is certain
    rad = np.zeros((200, 3), np.float32)
    rad[3] = (0.0, 5.0, 1.0)
    avg, rr = V.roulette(_vrl(rad))
    assert avg == F32(5.0) / F32(200.0) and rr[3] == 1.0 and np.count_nonzero(rr) == 1
    # avg == 0: 0 / 0 is NaN and f32::min returns the other operand
    avg, rr = V.roulette(_vrl(np.zeros((5, 3))))
    assert avg == 0.0 and (rr == 1.0).all()
    # a NaN channel is skipped by channel_max; an all-NaN radiance poisons the sum, and every rr is then 1
    avg, rr = V.roulette(_vrl([(np.nan, 2.0, 1.0), (2.0, 2.0, 2.0)]))
    assert avg == 2.0 and (rr == F32(0.01)).all()
    avg, rr = V.roulette(_vrl([(np.nan,) * 3, (2.0, 2.0, 2.0), (0.0, 0.0, 0.0)]))
    assert np.isnan(avg) and (rr == 1.0).all()
    # an infinite radiance: avg is infinite, inf / inf is NaN (rr = 1) and x / inf is 0
    avg, rr = V.roulette(_vrl([(np.inf, 0.0, 0.0), (2.0, 2.0, 2.0), (0.0, 0.0, 0.0)]))
    assert np.isposinf(avg) and rr.tolist() == [1.0, 0.0, 0.0]
    # negative radiance never passes (rr < 0 <= u), no VRL at all reports avg 0
    avg, rr = V.roulette(_vrl([(-1.0, -2.0, -3.0), (4.0, 0.0, 0.0)]))
    assert rr[0] < 0 and rr[1] > 0
    assert V.roulette(_vrl(np.zeros((0, 3))))[0] == 0.0


def test_zero_radiance_contributes_nothing_and_keeps_its_draws(built):
    """rr = 0 passes only on a draw of exactly 0; with avg == 0 every VRL passes (rr = 1), takes its three draws and adds black."""
    sd = scenes.cbox_medium(6, 4, 1.0)
    sc = orc.Scene(sd)
    surface = R.beam_words([(0.0, 1.0, 0.0)], 1.0, [(0.0, 0.6, 0.8)], [(1.0, 1.0, 1.0)])
    words = np.concatenate([surface, _vrl(np.zeros((4, 3)))])
    seeds = orc.block_seeds(1, 6, 4)
    img, st, detail = V.render(sc, sd, words, 1, seeds, 2, 0.3)
    assert st["vrl_accepted"] == 4 * st["camera_samples"] and st["rng_draws"] == st["camera_samples"] * (2 + 3 * 4)
    np.testing.assert_array_equal(detail["c"], detail["c_beams"])
    want, want_st = _scalar_render(sc, sd, words, 1, seeds, 2, 0.3)
    np.testing.assert_array_equal(img.view(np.uint32), want.view(np.uint32))
    assert want_st["rng_draws"] == st["rng_draws"]
