"""Oracle pinning, part 2: the deterministic transcendentals (oracle/detmath.h) against the platform
libm that rustlight itself would call through Rust's f32::{sin,cos,exp,ln,powf}.  CPU only."""
import ctypes
import ctypes.util

import numpy as np
import pytest

from oracle import orc
from rustlight_amd import abi

libm = ctypes.CDLL(ctypes.util.find_library("m"))
for f in ("sinf", "cosf", "expf", "logf", "acosf"):
    getattr(libm, f).restype = ctypes.c_float
    getattr(libm, f).argtypes = [ctypes.c_float]
libm.powf.restype = ctypes.c_float
libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]
libm.atan2f.restype = ctypes.c_float
libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]


def batch(fn, a, b=None):
    a = np.ascontiguousarray(a, np.float32)
    b = np.zeros_like(a) if b is None else np.ascontiguousarray(b, np.float32)
    out = np.zeros_like(a)
    orc.lib().orc_math_batch(fn, a.shape[0], abi.fptr(a), abi.fptr(b), abi.fptr(out))
    return out


def ulp_diff(x, y):
    xi = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
    yi = np.asarray(y, np.float32).view(np.int32).astype(np.int64)
    xi = np.where(xi < 0, -(xi & 0x7fffffff), xi)
    yi = np.where(yi < 0, -(yi & 0x7fffffff), yi)
    return np.abs(xi - yi)


def check(fn, name, a, b=None, min_equal=0.97):
    got = batch(fn, a, b)
    if b is None:
        ref = np.array([getattr(libm, name)(float(x)) for x in a], np.float32)
        exact = getattr(np, {"sinf": "sin", "cosf": "cos", "expf": "exp", "logf": "log", "acosf": "arccos"}[name])(a.astype(np.float64))
    else:
        ref = np.array([getattr(libm, name)(float(x), float(y)) for x, y in zip(a, b)], np.float32)
        exact = np.power(a.astype(np.float64), b.astype(np.float64)) if name == "powf" else np.arctan2(a.astype(np.float64), b.astype(np.float64))
    d = ulp_diff(got, ref)
    assert d.max() <= 1, (name, d.max())
    assert (d == 0).mean() >= min_equal, (name, (d == 0).mean())
    # and it is the correctly rounded value (f64 numpy result rounded to f32) almost everywhere
    cr = exact.astype(np.float32)
    assert (ulp_diff(got, cr) == 0).mean() >= 0.9999, name


def test_sin_cos(built):
    rng = np.random.default_rng(1)
    a = np.concatenate([rng.uniform(-np.pi, 2 * np.pi, 20000), rng.uniform(-0.8, 2.4, 20000), [0.0, 1e-8, -1e-8, np.pi / 4, np.pi / 2]]).astype(np.float32)
    check(0, "sinf", a, min_equal=0.97)
    check(1, "cosf", a, min_equal=0.97)


def test_exp_log_pow(built):
    rng = np.random.default_rng(2)
    check(2, "expf", rng.uniform(-60, 20, 20000).astype(np.float32), min_equal=0.97)
    check(3, "logf", np.exp(rng.uniform(-40, 40, 20000)).astype(np.float32), min_equal=0.97)
    x = rng.uniform(0, 1, 20000).astype(np.float32)
    y = rng.uniform(0.01, 200, 20000).astype(np.float32)
    check(4, "powf", x, y, min_equal=0.97)


def test_acos_atan2(built):
    rng = np.random.default_rng(3)
    check(5, "acosf", rng.uniform(-1, 1, 20000).astype(np.float32), min_equal=0.9)   # glibc acosf itself is only ~92 % correctly rounded
    check(6, "atan2f", rng.uniform(-3, 3, 20000).astype(np.float32), rng.uniform(-3, 3, 20000).astype(np.float32), min_equal=0.8)


def test_special_values(built):
    assert batch(2, [-200.0])[0] == 0.0 and np.isinf(batch(2, [100.0])[0])
    assert np.isneginf(batch(3, [0.0])[0]) and np.isnan(batch(3, [-1.0])[0])
    assert batch(4, [0.0], [2.0])[0] == 0.0 and batch(4, [0.3], [0.0])[0] == 1.0 and batch(4, [1.0], [77.0])[0] == 1.0
    assert np.isnan(batch(0, [np.inf])[0])


# ---- the oracle itself over the input sets of tests/math_sweep.py (every 61st f32 bit pattern + every pattern within 2^16 of each boundary; powf and atan2f on
# their crossed sets), against numpy's f64 function rounded to f32.  detmath.h promises the correctly rounded value except within ~1e-15 of a rounding boundary;
# the f64 result rounded to f32 is itself a double rounding, which is what the one ulp is for.  NaN, inf, zero and the sign of zero must sit where IEEE 754 /
# Rust's f32 methods put them: a result on the wrong side of any of these counts as a mismatch, never as an ulp distance.
from tests import math_sweep  # noqa: E402

# sinf / cosf reduce their argument with a two-term pi/2 (33 + 53 bits); the exhaustive CPU sweep (`math_sweep.py full --arm oracle --against f64 sinf cosf`) finds
# the smallest |x| with a result more than 1 ulp from the reference, and TRIG_ACCURATE_TO is the largest power of two below it.  Beyond it the two functions are
# defined by their restatement only (the device still has to equal the oracle there: test_gpu_math_sweep.py).
TRIG_ACCURATE_TO = 2.0 ** 23
MIN_EXACT = 0.9999        # the share of correctly rounded results the tests above already demand

DOMAIN = {
    "sinf": lambda fn, x, y: ~(np.abs(x) > np.float32(TRIG_ACCURATE_TO)),      # NaN and the inside; +-inf lie beyond and are checked in test_special_values
    "cosf": lambda fn, x, y: ~(np.abs(x) > np.float32(TRIG_ACCURATE_TO)),
    "expf": None, "logf": None, "acosf": None, "asinf": None,                  # every float
    "powf": lambda fn, x, y: ~np.signbit(x) | np.isnan(x),                     # x >= 0 (sign bit clear): see test_stated_deviations_of_powf for the rest
    "atan2f": lambda fn, x, y: ~(np.isinf(x) & np.isinf(y)),                   # see test_stated_deviation_of_atan2f
}


@pytest.mark.parametrize("name", list(DOMAIN))
def test_oracle_is_within_one_ulp_of_f64_over_the_sweep_sets(built, name):
    res = math_sweep.run(name, "default", arm="oracle", against="f64", select=DOMAIN[name])
    print(f"{name}: {res.inputs} inputs, worst {res.worst_ulp} ulp, exactly equal {res.exact_share:.8f}, zero signs {res.zero_sign}, {res.seconds:.1f} s")
    assert res.inputs > 1_000_000
    assert res.mismatches == 0, res.message()
    assert res.exact_share >= MIN_EXACT, res.message()


def test_trig_accuracy_stops_where_the_full_sweep_says(built):
    """Past TRIG_ACCURATE_TO the reduction has run out and nothing is claimed: the first miss of the exhaustive sweep, cos(8388654), the two a thinned look had
    found, cos(-8747493) and sin(16993104), are more than 1 ulp off, and sin(3e38) is not even in [-1, 1].  What the functions return out there is pinned by the
    device-vs-oracle sweep alone.  Up to the threshold itself they are accurate."""
    x = np.array([8388654.0, -8747493.0, 16993104.0], np.float32)
    assert x[0] > TRIG_ACCURATE_TO and 2 * TRIG_ACCURATE_TO > x[0]
    assert math_sweep.ulp_distance(batch(1, x[:2]), np.cos(x[:2].astype(np.float64)).astype(np.float32)).min() > 1
    assert math_sweep.ulp_distance(batch(0, x[2:]), np.sin(x[2:].astype(np.float64)).astype(np.float32))[0] > 1
    assert not abs(batch(0, [3.0e38])[0]) <= 1.0
    edge = np.array([TRIG_ACCURATE_TO, -TRIG_ACCURATE_TO], np.float32)
    assert math_sweep.ulp_distance(batch(0, edge), np.sin(edge.astype(np.float64)).astype(np.float32)).max() <= 1
    assert math_sweep.ulp_distance(batch(1, edge), np.cos(edge.astype(np.float64)).astype(np.float32)).max() <= 1


def test_stated_deviations_of_powf(built):
    """powf_det is powf for the bases rustlight produces: phong.rs raises a random number of [0, 1) and a cosine it has tested to be > 0.  Outside of that it
    deviates from IEEE 754 / Rust on purpose, and says so here: (1) x < 0 gives NaN for EVERY y other than 0, integers included (Rust: (-2)^2 = 4);
    (2) x = -0 is treated as +0: the result never carries a sign (IEEE: pow(-0, 3) = -0, pow(-0, -1) = -inf)."""
    ys = math_sweep.pow_exponents()
    nz = ys[ys != 0]
    for x in (-1.0, -0.5, -2.0, -3.0, -np.inf, -1e-45, -3.4028235e38):
        assert np.isnan(batch(4, np.full(nz.shape, x, np.float32), nz)).all(), x
        assert (batch(4, np.full(2, x, np.float32), np.array([0.0, -0.0], np.float32)) == 1.0).all()
    assert batch(4, [-2.0], [2.0]).view(np.uint32)[0] == 0x7fc00000 and np.power(np.float32(-2.0), np.float32(2.0)) == 4.0
    neg0, pos0 = batch(4, np.full(ys.shape, -0.0, np.float32), ys), batch(4, np.zeros(ys.shape, np.float32), ys)
    same = (neg0.view(np.uint32) == pos0.view(np.uint32)) | (np.isnan(neg0) & np.isnan(pos0))
    assert same.all()
    assert batch(4, [-0.0], [3.0]).view(np.uint32)[0] == 0 and np.isposinf(batch(4, [-0.0], [-1.0])[0])
    with np.errstate(all="ignore"):
        assert np.signbit(np.power(np.float32(-0.0), np.float32(3.0))) and np.isneginf(np.power(np.float32(-0.0), np.float32(-1.0)))


def test_stated_deviation_of_atan2f(built):
    """atan2f_det(+-inf, +-inf) is NaN (inf / inf) where IEEE 754 says +-pi/4, +-3pi/4.  Its one caller, to_spherical_coordinates (emitter.rs:318-326), passes
    two components of a normalised direction, which are finite; every other combination with an infinity is the IEEE value."""
    inf = np.float32(np.inf)
    for y in (inf, -inf):
        for x in (inf, -inf):
            assert np.isnan(batch(6, [y], [x])[0]) and np.isfinite(np.arctan2(y, x))
    y = np.array([1.0, -1.0, inf, -inf, inf, -inf, 0.0, -0.0], np.float32)
    x = np.array([inf, -inf, 1.0, 1.0, -0.0, 0.0, -inf, -inf], np.float32)
    assert np.array_equal(batch(6, y, x).view(np.uint32), np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("name", ["sinf", "cosf", "acosf", "asinf", "atan2f"])
def test_host_copy_of_the_shared_header_equals_oracle(built, name):
    """csrc/detmath_shared.h as the host compiler instantiates it (the copy scene.cpp and lighttree.cpp build the environment map's row weights and the light tree
    with; rl_debug_math_sweep, where = host) against oracle/detmath.h, bit for bit, over the default sets.  No GPU is touched."""
    res = math_sweep.run(name, "default", arm="host", against="oracle")
    print(f"{name}: {res.inputs} inputs, {res.mismatches} mismatches, {res.seconds:.1f} s")
    assert res.inputs > 1_000_000
    assert res.mismatches == 0, res.message()
