"""tests/pn_restatement.py held to itself and to closed forms, on the CPU: the literal scalar walk equals the vectorised render bit for bit; the equi-angular,
clamped and point-normal pdfs integrate to 1 over their range and cdf(sample(xi)) = xi; the truncated-exponential pdf integrates to 1 over [0, max_dist]; the
two definitions at the reference's panics on constructed numbers; the refused inputs' codes.  The closed forms are float64 and share nothing with the
restatement but the configuration."""
import numpy as np
import pytest

from oracle import orc
from rustlight_amd import api, scenes
from tests import pn_restatement as P

F32 = np.float32
W, H = 20, 17          # 2 x 2 blocks, both edges ragged


@pytest.mark.parametrize("use_aa", [True, False])
@pytest.mark.parametrize("strategy", P.STRATEGIES)
def test_scalar_walk_equals_vectorised(built, strategy, use_aa):
    """Both stream modes; the lights scene so that the data-dependent strategies meet both outcomes of the None test."""
    fr = P.frame("lights", W, H)
    seeds = orc.block_seeds(11, W, H)
    for mode, spp in ((api.STREAM_REFERENCE_ORDER, 2), (api.STREAM_PER_SAMPLE, 1)):
        img, st, det = P.render(fr, seeds, strategy, spp, use_aa, mode)
        img2, st2, det2 = P.render_walk(fr, seeds, strategy, spp, use_aa, mode)
        assert img.tobytes() == img2.tobytes() and st == st2, (strategy, use_aa, mode, st, st2)
        assert (det["some"], det["none"]) == (det2["some"], det2["none"])
        assert set(det["starts"]) == set(det2["starts"]) and all((det["starts"][b] == det2["starts"][b]).all() for b in det["starts"])
        assert st["camera_samples"] == W * H * spp and np.isfinite(img).all()
        if P.may_fail(strategy):
            assert det["some"] > 0 and det["none"] > 0, "both outcomes of the None test"
            extra = 3 if P.is_phase(strategy) else 1
            assert st["rng_draws"] == st["camera_samples"] * ((2 if use_aa else 0) + 4) + det["some"] * extra
        else:
            assert st["rng_draws"] == st["camera_samples"] * P.draws_per_sample(strategy, use_aa) and det["none"] == 0
        assert st["vertices"] == det["some"]


def test_reference_order_starts_follow_the_counts(built):
    """A pixel's start in its block's stream is the sum of the draws of the samples before it."""
    fr = P.frame("floating", W, H)
    seeds = orc.block_seeds(5, W, H)
    _, st, det = P.render(fr, seeds, "pn_ex", 2, True, api.STREAM_REFERENCE_ORDER)
    assert det["none"] > 0 and det["some"] > 0
    total = 0
    for b, starts in det["starts"].items():
        assert starts[0] == 0 and (np.diff(starts) >= 2 * 6).all() and (np.diff(starts) <= 2 * 7).all()
        _, _, _, cnt, walk_starts = P.walk_block(fr, b, int(seeds[b]), "pn_ex", 2, True)
        assert (walk_starts == starts).all()
        total += int(cnt["draws"].sum())
    assert total == st["rng_draws"]


# ---- closed forms: a ray o + t d with d = +x from the origin, a light point at (delta, D, 0) with normal n in the xy plane
def _config(delta, dist, n, max_dist):
    o = np.zeros((1, 3), F32)
    d = np.asarray([[1.0, 0.0, 0.0]], F32)
    pos = np.asarray([[delta, dist, 0.0]], F32)
    nrm = np.asarray([n], F32)
    nrm = nrm / np.linalg.norm(nrm)
    has_max = np.asarray([max_dist is not None])
    md = np.asarray([max_dist if max_dist is not None else 0.0], F32)
    return has_max, md, o, d, pos, nrm.astype(F32)


CONFIGS = {
    "facing, bounded": (1.0, 0.7, (0.0, -1.0, 0.0), 3.0),
    "plane cuts the ray": (1.0, 0.7, (-0.6, -0.8, 0.0), 3.0),           # the light's plane crosses the ray in front of the origin: one side is clamped away
    "origin behind the light": (1.0, 0.7, (0.8, -0.6, 0.0), 3.0),      # p_dot_n > 0: theta_a is the clamp
    "parallel ray": (0.5, 1.2, (0.0, -1.0, 0.0), 2.0),                 # d . n = 0: no clamp
    "unbounded ray": (1.0, 0.7, (-0.6, -0.8, 0.0), None),              # theta_b = pi / 2 - 1e-5 unless clamped
}
XI = np.asarray([0.001, 0.1, 0.25, 0.5, 0.75, 0.9, 0.999], F32)


def _rep(x, n):
    return np.repeat(x, n, axis=0)


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("strategy", ["eq_ex", "eq_clamped_ex", "pn_ex"])
def test_angular_pdfs_integrate_to_one_and_invert(built, name, strategy):
    has_max, md, o, d, pos, nrm = _config(*CONFIGS[name])
    s, ok = P.make_sampler(strategy, has_max, md, o, d, pos, nrm)
    assert ok[0], (name, strategy)
    ta, tb, delta, dl = (float(s[k][0]) for k in ("theta_a", "theta_b", "delta", "d_l"))
    assert ta < tb
    n = XI.shape[0]
    sn = {k: _rep(v, n) for k, v in s.items()}
    if strategy == "pn_ex":
        t, pdf = P.sample_point_normal(sn, XI)
        a, b = float(s["a"][0]), float(s["b"][0])
        ang = lambda th: a * np.cos(th) + b * np.sin(th)                                     # normalised: its integral over [ta, tb] is 1
        cdf = lambda th: a * (np.sin(th) - np.sin(ta)) - b * (np.cos(th) - np.cos(ta))
    else:
        t, pdf = P.sample_equiangular(sn, _rep(has_max, n), _rep(md, n), XI)
        ang = lambda th: np.full_like(th, 1.0 / (tb - ta))
        cdf = lambda th: (th - ta) / (tb - ta)
    # the pdf over the angle integrates to 1 (midpoint rule in float64), and over the distance with the Jacobian D / (D^2 + (t - delta)^2)
    th = ta + (np.arange(200000) + 0.5) * (tb - ta) / 200000
    assert abs(ang(th).sum() * (tb - ta) / 200000 - 1.0) < 2e-5, (name, strategy)
    tt = delta + dl * np.tan(th)
    jac = dl / (dl * dl + (tt - delta) ** 2)
    dt = dl / np.cos(th) ** 2 * (tb - ta) / 200000
    assert abs((ang(th) * jac * dt).sum() - 1.0) < 2e-5
    # cdf(sample(xi)) = xi and the returned pdf is the density at the returned distance
    theta = np.arctan((t.astype(np.float64) - delta) / dl)
    inside = (t > 0) & (True if not has_max[0] else t < md[0])                               # the equi-angular sample clamps its distance to the ray
    assert inside.any()
    assert np.allclose(cdf(theta[inside]), XI[inside], atol=5e-4), (name, strategy, cdf(theta), XI)
    want = ang(theta) * dl / (dl * dl + (t.astype(np.float64) - delta) ** 2)
    assert np.allclose(pdf[inside], want[inside], rtol=2e-3), (name, strategy)


def test_clamp_moves_the_right_end(built):
    """The light's plane cuts the ray at t_hit: with the origin in front of the light the far end is clamped, behind it the near end."""
    for name, end in (("plane cuts the ray", "theta_b"), ("origin behind the light", "theta_a")):
        has_max, md, o, d, pos, nrm = _config(*CONFIGS[name])
        plain, _ = P.make_sampler("eq_ex", has_max, md, o, d, pos, nrm)
        clamped, ok = P.make_sampler("eq_clamped_ex", has_max, md, o, d, pos, nrm)
        other = "theta_a" if end == "theta_b" else "theta_b"
        assert ok[0] and clamped[other][0] == plain[other][0] and clamped[end][0] != plain[end][0]
        t_hit = float(np.dot((pos - o)[0], nrm[0]) / np.dot(d[0], nrm[0]))
        assert abs(np.tan(float(clamped[end][0])) * float(plain["d_l"][0]) + float(plain["delta"][0]) - t_hit) < 1e-4
    # the whole ray lies behind the light's plane and runs away from it (d . n <= 0 and (pos - o) . n >= 0): None
    has_max, md, o, d, pos, nrm = _config(1.0, 0.7, (-0.28, 0.96, 0.0), 3.0)
    assert not P.make_sampler("eq_clamped_ex", has_max, md, o, d, pos, nrm)[1][0]
    assert not P.make_sampler("pn_ex", has_max, md, o, d, pos, nrm)[1][0]
    # a point light's zero normal: always None
    assert not P.make_sampler("pn_ex", has_max, md, o, d, pos, np.zeros((1, 3), F32))[1][0]
    assert not P.make_sampler("eq_clamped_phase", has_max, md, o, d, pos, np.zeros((1, 3), F32))[1][0]


@pytest.mark.parametrize("sigma", [((1.0,) * 3, (0.0,) * 3), P.COLOURED, ((0.2, 0.7, 2.5), (0.0, 0.1, 0.4))])
def test_truncated_exponential_integrates_to_one(built, sigma):
    med = P.Medium(scenes.Medium(sigma[1], sigma[0], scenes.PHASE_ISOTROPIC, 0.0))
    st = med.sigma_t.astype(np.float64)
    for v in (0.3, 2.0, 9.0):
        t = (np.arange(200000) + 0.5) * v / 200000
        pdf = (st[None, :] * np.exp(-st[None, :] * t[:, None]) / (1.0 - np.exp(-st[None, :] * v))).mean(axis=1)
        assert abs(pdf.sum() * v / 200000 - 1.0) < 1e-6
        n = XI.shape[0]
        ts, ps, ok = P.sample_transmittance(med, np.ones(n, bool), np.full(n, v, F32), XI)
        assert ok.all() and (ts >= 0).all() and (ts <= v * (1 + 1e-6)).all()
        want = (st[None, :] * np.exp(-st[None, :] * ts.astype(np.float64)[:, None]) / (1.0 - np.exp(-st[None, :] * v))).mean(axis=1)
        assert np.allclose(ps, want, rtol=1e-5)
        # the channel is picked by thirds of xi and the rest of xi inverts that channel's cdf
        comp = np.minimum((XI.astype(np.float64) * 3).astype(int), 2)
        u = XI.astype(np.float64) * 3 - comp
        assert np.allclose((1 - np.exp(-st[comp] * ts)) / (1 - np.exp(-st[comp] * v)), u, atol=2e-5)
    # unbounded: the free path's own density
    ts, ps, ok = P.sample_transmittance(med, np.zeros(XI.shape[0], bool), np.zeros(XI.shape[0], F32), XI)
    assert ok.all() and np.allclose(ps, (st[None, :] * np.exp(-st[None, :] * ts.astype(np.float64)[:, None])).mean(axis=1), rtol=1e-5)


def test_the_two_defined_panics(built):
    # (1) both atans saturate: the light far beyond a short ray, almost on its line
    has_max, md, o, d, pos, nrm = _config(1.0e6, 1.0e-3, (0.0, -1.0, 0.0), 2.0)
    s, ok = P.make_sampler("eq_ex", has_max, md, o, d, pos, nrm)
    assert s["theta_a"][0] == s["theta_b"][0] and not ok[0]
    # ... and such a sample takes its usual draws and adds zero
    fr = P.frame("box", W, H)
    taken = []

    def draw():
        taken.append(len(taken))
        return np.asarray([0.5], F32)

    real = P.make_sampler
    try:
        P.make_sampler = lambda *a: (real(*a)[0], np.zeros(1, bool))
        for strategy, count in (("eq_ex", 7), ("eq_phase", 9)):
            del taken[:]
            rad, cnt = P.evaluate(fr, strategy, True, np.asarray([3]), np.asarray([4]), draw)
            assert len(taken) == count == int(cnt["draws"][0]) and not rad.any() and cnt["vertices"][0] == 0 and cnt["shadow"][0] == 0
    finally:
        P.make_sampler = real
    # (2) the free path leaves an unbounded ray: a medium thin enough for the distance to overflow
    thin = P.Medium(scenes.Medium((0.0,) * 3, (1e-39,) * 3, scenes.PHASE_ISOTROPIC, 0.0))
    t, pdf, ok = P.sample_transmittance(thin, np.zeros(1, bool), np.zeros(1, F32), np.asarray([0.2], F32))
    assert not ok[0]
    t, pdf, ok = P.sample_transmittance(thin, np.ones(1, bool), np.ones(1, F32), np.asarray([0.2], F32))
    assert ok[0]


def test_refused_inputs_and_their_codes(built):
    def code(f, *a, **k):
        with pytest.raises(P.Refused) as e:
            f(*a, **k)
        return e.value.code

    assert code(P.check_scene, scenes.cbox(W, H)) == P.RL_ERR_UNSUPPORTED                                        # no medium
    sd = P.scene("box", W, H); sd.use_ats = True
    assert code(P.check_scene, sd) == P.RL_ERR_UNSUPPORTED
    sd = P.scene("box", W, H); sd.lights.append({"type": "directional", "a": (0.0, -1.0, 0.0), "intensity": (1.0, 1.0, 1.0)})
    assert code(P.check_scene, sd) == P.RL_ERR_UNSUPPORTED
    sd = P.scene("box", W, H); sd.meshes[-1].emission = None
    assert code(P.check_scene, sd) == P.RL_ERR_NO_EMITTER
    assert code(P.check_params, "tr_ex", 0, 0, 0, 1) == P.RL_ERR_INVALID_ARGUMENT
    assert code(P.check_params, "pn_best_ex", 1, 0, 0, 1) == P.RL_ERR_INVALID_ARGUMENT
    assert code(P.check_params, "tr_ex", 1, api.STREAM_STRATIFIED, 0, 1) == P.RL_ERR_UNSUPPORTED
    assert code(P.check_params, "tr_ex", 1, 0, 2, 2) == P.RL_ERR_INVALID_ARGUMENT
    assert code(P.check_params, "eq_phase", (1 << 32) // (256 * 9) + 1, 0, 0, 1) == P.RL_ERR_UNSUPPORTED           # 256 * spp * D > 2^32 - 1
    P.check_params("eq_phase", (1 << 32) // (256 * 9) - 1, 0, 0, 1)
    P.check_params("pn_ex", 1 << 24, 0, 0, 1)                                                                     # no jump, no limit
    P.check_params("eq_phase", 1 << 24, api.STREAM_PER_SAMPLE, 0, 1)
