"""A float64 quadrature of what the virtual ray lights estimate, the yardstick of tests/test_vrl_quadrature.py and tests/test_gpu_vrl_quadrature.py (a plain
module: `from tests import vrl_quadrature`).  It shares no code with the kernels or with tests/vrl_restatement.py except the oracle's `visible`.

For a camera ray (o, d, tnear, tfar) and a VRL (a, b, length, radiance) with roulette probability 1, the estimator of
src/integrators/explicit/vol_primitives.rs:201-253 draws t_cam and t_vrl uniformly and weighs by the inverse density, so its expectation is the pair integral

    L = radiance / n_paths * (sigma_s / 4 pi)^2 * Int_tnear^tfar dt_cam Int_0^length dt_vrl  V(p_cam, p_vrl) e^(-sigma_t t_cam) e^(-sigma_t r) / r^2,
    p_cam = o + d t_cam,  p_vrl = a + b t_vrl,  r = |p_vrl - p_cam|,

written here from the rendering equation's two-vertex form: two scattering events, each sigma_s times the isotropic phase function 1 / 4 pi, the geometry term
1 / r^2 between two points of a medium, and the transmittances along the camera segment and the connection.  Both integrals are Gauss-Legendre rules of the
same order on the whole interval; the error estimate is the difference to the rule of half the order (pair_integral_with_error), and the closed form of a
short VRL in a near-vacuum checks the rule from outside."""
import numpy as np

TNEAR = 1e-4


def pair_integral(sc, vrls, o, d, tfar, sigma_s, sigma_t, order, n_paths=1):
    """L [n_rays, 3] float64.  vrls: [(a [3], b [3], length, radiance [3])]; o, d [n_rays, 3]; tfar [n_rays] (finite)."""
    o, d, tfar = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3), np.asarray(tfar, np.float64).reshape(-1)
    assert np.isfinite(tfar).all()
    sigma_s, sigma_t = np.asarray(sigma_s, np.float64), np.asarray(sigma_t, np.float64)
    x, w = np.polynomial.legendre.leggauss(order)
    half = 0.5 * (tfar - TNEAR)
    t_cam = TNEAR + half[:, None] * (x[None, :] + 1.0)                    # [n, q]
    w_cam = half[:, None] * w[None, :]
    p_cam = o[:, None, :] + d[:, None, :] * t_cam[:, :, None]             # [n, q, 3]
    n = o.shape[0]
    out = np.zeros((n, 3))
    for a, b, length, radiance in vrls:
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        t_vrl = 0.5 * length * (x + 1.0)
        w_vrl = 0.5 * length * w
        p_vrl = a[None, :] + b[None, :] * t_vrl[:, None]                  # [q, 3]
        delta = p_vrl[None, None, :, :] - p_cam[:, :, None, :]            # [n, q, q, 3]
        r2 = (delta * delta).sum(axis=3)
        r = np.sqrt(r2)
        pc = np.broadcast_to(p_cam[:, :, None, :], delta.shape).reshape(-1, 3)
        pv = np.broadcast_to(p_vrl[None, None, :, :], delta.shape).reshape(-1, 3)
        vis = sc.visible(pc, pv).reshape(r.shape).astype(np.float64)
        weight = vis * w_cam[:, :, None] * w_vrl[None, None, :] / r2
        for ch in range(3):
            f = np.exp(-sigma_t[ch] * (t_cam[:, :, None] + r))
            out[:, ch] += radiance[ch] * (sigma_s[ch] / (4.0 * np.pi)) ** 2 * (weight * f).sum(axis=(1, 2))
    return out / float(n_paths)


def pair_integral_with_error(sc, vrls, o, d, tfar, sigma_s, sigma_t, order, n_paths=1):
    """(L at `order` [n_rays, 3], |L(order) - L(order / 2)| [n_rays, 3])."""
    fine = pair_integral(sc, vrls, o, d, tfar, sigma_s, sigma_t, order, n_paths)
    coarse = pair_integral(sc, vrls, o, d, tfar, sigma_s, sigma_t, order // 2, n_paths)
    return fine, np.abs(fine - coarse)


def short_vrl_closed_form(vrl, o, d, tfar, sigma_s, n_paths=1):
    """The pair integral of a VRL short against its distance h from the ray, in a vacuum, everything visible: with the VRL's middle m, s = (m - o) . d the foot
    of its perpendicular and h = |m - o - s d|, Int dt / (h^2 + (t - s)^2) = (theta_b - theta_a) / h with tan(theta) = (t - s) / h at both ends of the ray;
    times the VRL's length."""
    a, b, length, radiance = vrl
    m = np.asarray(a, np.float64) + np.asarray(b, np.float64) * (0.5 * length)
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    s = float((m - o) @ d)
    h = float(np.linalg.norm(m - o - s * d))
    theta_a, theta_b = np.arctan((TNEAR - s) / h), np.arctan((float(tfar) - s) / h)
    return np.asarray(radiance, np.float64) * (np.asarray(sigma_s, np.float64) / (4.0 * np.pi)) ** 2 * ((theta_b - theta_a) / h) * length / float(n_paths)
