"""The deterministic math layer over (nearly) every float.  Three texts of the same functions exist — oracle/detmath.h (g++), csrc/detmath_shared.h +
kernels/devmath.hip.h on the device (hipcc) and the host compiler's copy of detmath_shared.h that builds the light tree — and the project's claim "bit-identical
to the oracle" holds only while they are one function.  `run(name, ...)` evaluates one function family on one of them (`arm`) over an input set and compares it

    against = "oracle": bit for bit with the oracle (`view(np.uint32)` equal; -0 and +0 differ).  The one exception: where both results are NaN the payload
                        (and sign) of the NaN is not compared.  div_rn / sqrt_rn / a * b + a have no oracle text: their reference is IEEE-754 itself, i.e.
                        numpy's f32 divide, sqrt and multiply-then-add (two roundings).
    against = "f64":    in ulps with numpy's f64 function rounded to f32, the high-precision reference (that rounding is a double rounding: hence "<= 1 ulp").

Input sets ("default": what the suites run; "full": by hand) are lists of arithmetic progressions of f32 bit patterns, so the device generates them itself
(rl_debug_math_sweep) and nothing but the second argument of a binary function is ever uploaded:
    unary    every STRIDE-th bit pattern (61: ~70 M values, every binade ~137 k times) plus every pattern within 2^16 of the boundaries listed in `_windows`;
             full = all 2^32.
    powf     x: 2^16 evenly spaced patterns of (0, 1] + the 2^12 patterns nearest 0+, the denormal border and 1-;  y: 1/(n+1), 2/(n+1), n for n = 0 ... 4096 and
             64 log-spaced n up to 1e6, +-0, +-0.5, +-1, +-2, +-inf, NaN;  and x in {+-0, 1, +inf, NaN, x < 0} crossed with those y.
    atan2f   E x E for the edge set E (+-0, +-smallest denormal, +-FLT_MIN, +-1, +-FLT_MAX, +-inf, NaN, 2^10 random patterns), and for x in
             {+-0, +-1, +-FLT_MIN, +-inf} every y of the unary set.
    div_rn   the unary sets for 1 / x, x / c and c / x (c = 3, pi, 255, 1e-20); E x E; 2^26 random bit-pattern pairs; 2^22 pairs whose quotient is denormal.
    mul_add  E x E; 2^26 random pairs; 2^22 pairs with a denormal product.

By hand, one process, sequentially:   python tests/math_sweep.py full|default [--arm device|host|oracle] [--against oracle|f64] [--stride N] [function ...]
prints per function: inputs, mismatches (or worst ulp / share of exact results), seconds."""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from oracle import orc
from rustlight_amd import abi, api

THREADS = min(16, os.cpu_count() or 1)     # the oracle is serial; chunks run side by side (ctypes releases the GIL).  Never more than 16.
CHUNK = 1 << 20                            # values per call: 4 MB per array, so that 16 chunks in flight with their f64 temporaries stay under a GB
STRIDE = 61                                # default thinning of the unary sets (a prime; the boundary windows are never thinned)
WINDOW = 1 << 16
FUNCTIONS = ("sinf", "cosf", "expf", "logf", "acosf", "asinf", "sqrt_rn", "div_rn", "powf", "atan2f", "mul_add")
ORACLE_CODE = {"sinf": 0, "cosf": 1, "expf": 2, "logf": 3, "powf": 4, "acosf": 5, "atan2f": 6, "asinf": 7}      # orc_math_batch
F64 = {"sinf": np.sin, "cosf": np.cos, "expf": np.exp, "logf": np.log, "acosf": np.arccos, "asinf": np.arcsin, "powf": np.power, "atan2f": np.arctan2}
DIV_CONSTANTS = (3.0, float(np.float32(np.pi)), 255.0, 1e-20)


def bits(x):
    return int(np.array(x, np.float32).view(np.uint32))


def f32(b):
    return np.array(b, np.uint32).view(np.float32)


def progression(first, stride, n, period=0):
    i = np.arange(n, dtype=np.uint32)
    if period:
        i %= np.uint32(period)
    return (i * np.uint32(stride & 0xffffffff) + np.uint32(first & 0xffffffff)).view(np.float32)      # uint32 arithmetic wraps, as the hook's does


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# input sets
COMMON_EDGES = [0x00000000, 0x80000000, 0x00800000, 0x80800000, 0x3f800000, 0xbf800000, 0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000,
                0x7fc00000, 0xffc00000, 0x7fa00000, 0xffa00000, 0x7fffffff, 0xffffffff]      # +-0, FLT_MIN, +-1, +-FLT_MAX, +-inf, quiet / signalling NaN, all ones


def _windows(name):
    """Bit patterns whose 2^16 neighbours on either side are never thinned."""
    w = list(COMMON_EDGES)
    if name == "expf":      # ln(FLT_MAX), ln(FLT_MIN), ln(2^-150), and the two cut-offs of the text itself
        w += [bits(88.72284), bits(-87.33654), bits(-103.97208), bits(89.0), bits(-104.0)]
    if name in ("sinf", "cosf"):
        for k in range(1, 65):
            w += [bits(k * np.pi / 2), bits(-k * np.pi / 2)]
        for v in (2.0 ** 20, 8.7e6, 2.0 ** 24, 2.0 ** 31):
            w += [bits(v), bits(-v)]
    return w


def unary_segments(name, mode, stride=STRIDE):
    """[(first_bits, stride, n)]: a cover of the set, windows merged so that no pattern is evaluated twice by them."""
    if mode == "full":
        return [(0, 1, 1 << 32)]
    iv = []
    for c in _windows(name):
        lo, hi = c - WINDOW, c + WINDOW
        iv += [(max(lo, 0), min(hi, 0xffffffff))]
        if lo < 0: iv.append((lo + (1 << 32), 0xffffffff))
        if hi > 0xffffffff: iv.append((0, hi - (1 << 32)))
    if name == "logf":
        iv.append((0, 0x00800000))      # every denormal input
    iv.sort()
    merged = [list(iv[0])]
    for lo, hi in iv[1:]:
        if lo <= merged[-1][1] + 1: merged[-1][1] = max(merged[-1][1], hi)
        else: merged.append([lo, hi])
    return [(0, stride, ((1 << 32) + stride - 1) // stride)] + [(lo, 1, hi - lo + 1) for lo, hi in merged]


def edge_set():
    e = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00800000, 0x80800000, 0x3f800000, 0xbf800000, 0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000, 0x7fc00000]
    return np.concatenate([np.array(e, np.uint32), np.random.default_rng(7).integers(0, 1 << 32, 1 << 10, dtype=np.uint64).astype(np.uint32)]).view(np.float32)


def pow_exponents():
    n = np.concatenate([np.arange(0, 4097), np.unique(np.round(np.logspace(np.log10(4097.0), 6.0, 64)))]).astype(np.float32)
    one, two = np.float32(1.0), np.float32(2.0)
    with np.errstate(all="ignore"):
        y = np.concatenate([one / (n + one), two / (n + one), n, np.array([0.0, -0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, np.inf, -np.inf, np.nan], np.float32)])
    _, idx = np.unique(y.view(np.uint32), return_index=True)
    return y[np.sort(idx)]


POW_X_SEGMENTS = [(16256, 16256, 1 << 16),                       # 2^16 evenly spaced patterns of (0, 1]: the last one is 0x3f800000
                  (1, 1, 1 << 12), (0x00800000 - (1 << 11), 1, 1 << 12), (0x3f800000 - (1 << 12), 1, 1 << 12)]
POW_X_SPECIAL = [0.0, -0.0, 1.0, np.inf, np.nan, -1.0, -0.5, -2.0, -3.0, -np.inf, -1e-45, -3.4028235e38]
ATAN2_FIXED_X = [0.0, -0.0, 1.0, -1.0, 1.17549435e-38, -1.17549435e-38, np.inf, -np.inf]


class Job:
    """out[i] = fn(g_i, b_i), or fn(b_i, g_i) with swap; g = progression(first, stride, n, period); b None, one number or n numbers."""
    __slots__ = ("fn", "first", "stride", "period", "n", "b", "swap")

    def __init__(self, fn, first, stride, n, b=None, swap=False, period=0):
        self.fn, self.first, self.stride, self.period, self.n, self.b, self.swap = fn, first, stride, period, n, b, swap

    def args(self):
        g = progression(self.first, self.stride, self.n, self.period)
        if self.b is None:
            return g, None
        b = np.ascontiguousarray(np.broadcast_to(np.asarray(self.b, np.float32), (self.n,)))
        return (b, g) if self.swap else (g, b)


def _chunked(fn, segs, b=None, swap=False):
    for first, stride, n in segs:
        for o in range(0, n, CHUNK):
            yield Job(fn, first + o * stride, stride, min(CHUNK, n - o), b, swap)


def _crossed(fn, values, seconds):
    for v in values:      # one constant first argument against the whole second set
        yield Job(fn, bits(v), 0, len(seconds), seconds)


def _random_pairs(fn, log2n, seed):
    """g walks all 2^32 patterns in the order of an odd (golden-ratio) step from a seeded start; b is seeded random bit patterns."""
    rng = np.random.default_rng(seed)
    first = int(rng.integers(0, 1 << 32))
    for o in range(0, 1 << log2n, CHUNK):
        yield Job(fn, first + o * 0x9e3779b1, 0x9e3779b1, CHUNK, rng.integers(0, 1 << 32, CHUNK, dtype=np.uint64).astype(np.uint32).view(np.float32))


def _denormal_pairs(fn, seed):
    rng = np.random.default_rng(seed)
    n = 1 << 22
    if fn == "div_rn":      # a over 2^-100 ... 2^-60, b = a / t for a random denormal t of either sign: the quotient lands next to t
        first, stride = 0x0d800000, 80
        t = (rng.integers(1, 1 << 23, n, dtype=np.uint64).astype(np.uint32) | (rng.integers(0, 2, n, dtype=np.uint64).astype(np.uint32) << np.uint32(31))).view(np.float32)
        b = (progression(first, stride, n).astype(np.float64) / t.astype(np.float64)).astype(np.float32)
    else:                   # a over the denormals and the first two normal binades, b in (-2, 2): product and sum stay down there
        first, stride = 1, 4
        b = rng.uniform(-2.0, 2.0, n).astype(np.float32)
    for o in range(0, n, CHUNK):
        yield Job(fn, first + o * stride, stride, min(CHUNK, n - o), b[o:o + CHUNK])


def jobs(name, mode="default", stride=STRIDE):
    if name in ("sinf", "cosf", "expf", "logf", "acosf", "asinf", "sqrt_rn"):
        yield from _chunked(name, unary_segments(name, mode, stride))
    elif name == "div_rn":
        segs = unary_segments(name, mode, stride)
        yield from _chunked(name, segs, 1.0, swap=True)      # the reciprocal
        for c in DIV_CONSTANTS:
            yield from _chunked(name, segs, c)
            yield from _chunked(name, segs, c, swap=True)
        yield from binary_jobs(name)
    elif name == "mul_add":
        yield from binary_jobs(name)
    elif name == "atan2f":
        e = edge_set()
        yield from _crossed(name, e, e)
        for x in ATAN2_FIXED_X:
            yield from _chunked(name, unary_segments(name, mode, stride), x)
    elif name == "powf":
        ys = pow_exponents()
        for first, st, period in POW_X_SEGMENTS:
            per_call = max(1, CHUNK // period)
            for o in range(0, len(ys), per_call):
                y = ys[o:o + per_call]
                yield Job(name, first, st, period * len(y), np.repeat(y, period), period=period)
        yield from _crossed(name, POW_X_SPECIAL, ys)
    else:
        raise KeyError(name)


def binary_jobs(name):
    """div_rn / mul_add on pairs: E x E, 2^26 random pairs, 2^22 pairs with a denormal quotient / product."""
    e = edge_set()
    yield from _crossed(name, e, e)
    yield from _random_pairs(name, 26, seed=11)
    yield from _denormal_pairs(name, seed=12)


def discriminating_pairs(name):
    """How many pairs of the binary set tell the contract from its cheaper neighbour — mul_add: a fused multiply-add (f64 product + add, rounded once) from
    two roundings; div_rn: a * (float)(1.0 / b) from a / b.  A set without such pairs could not see the difference."""
    def count(job):
        a, b = job.args()
        with np.errstate(all="ignore"):
            if name == "mul_add":
                ref = a * b + a
                alt = (a.astype(np.float64) * b.astype(np.float64) + a.astype(np.float64)).astype(np.float32)
            else:
                ref = a / b
                alt = a * (1.0 / b.astype(np.float64)).astype(np.float32)
        return int(np.count_nonzero(_differ(alt, ref)))
    with ThreadPoolExecutor(THREADS) as ex:
        return sum(ex.map(count, binary_jobs(name)))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the three texts and the two references
def _oracle(fn, x, y):
    with np.errstate(all="ignore"):
        if fn == "sqrt_rn": return np.sqrt(x)
        if fn == "div_rn": return x / y
        if fn == "mul_add": return x * y + x      # f32 arrays: a rounded product, then a rounded sum
    out = np.empty_like(x)
    orc.lib().orc_math_batch(ORACLE_CODE[fn], x.shape[0], abi.fptr(x), abi.fptr(x if y is None else y), abi.fptr(out))
    return out


def _f64(fn, x, y):
    with np.errstate(all="ignore"):
        if fn == "sqrt_rn": return np.sqrt(x.astype(np.float64)).astype(np.float32)
        if fn == "div_rn": return (x.astype(np.float64) / y.astype(np.float64)).astype(np.float32)
        if y is None: return F64[fn](x.astype(np.float64)).astype(np.float32)
        return F64[fn](x.astype(np.float64), y.astype(np.float64)).astype(np.float32)


def _hook(job, where):
    return api.math_sweep(job.fn, job.first, job.stride, job.n, job.b, job.swap, job.period, where)


def _differ(got, ref):
    """Bit for bit; the payload of a NaN that both sides return is the one thing not compared."""
    return (got.view(np.uint32) != ref.view(np.uint32)) & ~(np.isnan(got) & np.isnan(ref))


def ulp_distance(got, ref):
    """Distance in f32 steps on the ordered number line (+-0 coincide); 0 where both are NaN, 2^32 where only one is."""
    gi, ri = got.view(np.int32).astype(np.int64), ref.view(np.int32).astype(np.int64)
    gi = np.where(gi < 0, -(gi & 0x7fffffff), gi)
    ri = np.where(ri < 0, -(ri & 0x7fffffff), ri)
    d = np.abs(gi - ri)
    gn, rn = np.isnan(got), np.isnan(ref)
    d[gn & rn] = 0
    d[gn != rn] = 1 << 32
    return d


class Result:
    def __init__(self, name, arm, against):
        self.name, self.arm, self.against = name, arm, against
        self.inputs = self.mismatches = self.exact = self.over_one = self.zero_sign = 0
        self.worst_ulp = 0
        self.first_over_one = np.inf      # smallest |first argument| with a result more than 1 ulp from the reference
        self.examples = []                # (first argument bits, second argument bits or None, got bits, reference bits)
        self.seconds = 0.0

    def add(self, x, y, got, ref, keep=None):
        if keep is not None:
            x, got, ref = x[keep], got[keep], ref[keep]
            y = None if y is None else y[keep]
        self.inputs += x.shape[0]
        if self.against == "oracle":
            bad = _differ(got, ref)
        else:
            d = ulp_distance(got, ref)
            zs = (got == 0) & (ref == 0) & (np.signbit(got) != np.signbit(ref))
            self.zero_sign += int(np.count_nonzero(zs))
            self.exact += int(np.count_nonzero((d == 0) & ~zs))
            self.worst_ulp = max(self.worst_ulp, int(d.max(initial=0)))
            bad = (d > 1) | zs
            self.over_one += int(np.count_nonzero(d > 1))
            if (d > 1).any():
                self.first_over_one = min(self.first_over_one, float(np.abs(x[d > 1]).astype(np.float64).min()))
        k = int(np.count_nonzero(bad))
        self.mismatches += k
        if k and len(self.examples) < 8:
            for i in np.flatnonzero(bad)[:8 - len(self.examples)]:
                self.examples.append((int(x.view(np.uint32)[i]), None if y is None else int(y.view(np.uint32)[i]), int(got.view(np.uint32)[i]), int(ref.view(np.uint32)[i])))

    def merge(self, o):
        for k in ("inputs", "mismatches", "exact", "over_one", "zero_sign"):
            setattr(self, k, getattr(self, k) + getattr(o, k))
        self.worst_ulp, self.first_over_one = max(self.worst_ulp, o.worst_ulp), min(self.first_over_one, o.first_over_one)
        self.examples += o.examples[:8 - len(self.examples)]

    @property
    def exact_share(self):
        return self.exact / max(self.inputs, 1)

    def message(self):
        ex = ", ".join("(" + ", ".join("-" if v is None else f"{v:08x}" for v in e) + ")" for e in self.examples)
        s = f"{self.name}: {self.arm} vs {self.against}: {self.mismatches} of {self.inputs} inputs differ"
        if self.against == "f64":
            s += f" by more than 1 ulp or in the sign of zero (worst {self.worst_ulp} ulp, {self.zero_sign} zero signs, exactly equal {self.exact_share:.8f})"
        return s + (f"; first (input bits, second input bits, {self.arm} bits, {self.against} bits): {ex}" if ex else "")


def run(name, mode="default", arm="device", against="oracle", stride=STRIDE, select=None, verbose=False):
    """One function family `name` of FUNCTIONS on `arm` ("device": the kernels' build through rl_debug_math_sweep; "host": the host compiler's copy of
    detmath_shared.h, no GPU; "oracle": oracle/detmath.h) against "oracle" (bits) or "f64" (ulps).  select(fn, x, y) -> bool mask restricts what is counted
    (the accuracy claims have domains).  Device calls are made one at a time from this thread; everything else runs in the pool."""
    assert arm in ("device", "host", "oracle") and against in ("oracle", "f64") and arm != against
    res = Result(name, arm, against)
    t0 = time.perf_counter()

    def work(job, got):
        x, y = job.args()
        if got is None:
            got = _hook(job, api.MATH_ON_HOST) if arm == "host" else _oracle(job.fn, x, y)
        ref = _oracle(job.fn, x, y) if against == "oracle" else _f64(job.fn, x, y)
        part = Result(name, arm, against)
        part.add(x, y, got, ref, None if select is None else select(job.fn, x, y))
        return part

    with ThreadPoolExecutor(THREADS) as ex:
        pending = []
        for job in jobs(name, mode, stride):
            pending.append(ex.submit(work, job, _hook(job, api.MATH_ON_DEVICE) if arm == "device" else None))
            while len(pending) >= 2 * THREADS:
                res.merge(pending.pop(0).result())
        for f in pending:
            res.merge(f.result())
    res.seconds = time.perf_counter() - t0
    if verbose:
        print(f"{name:8s} {mode:7s} {arm} vs {against}: inputs {res.inputs}, mismatches {res.mismatches}"
              + (f", worst {res.worst_ulp} ulp, exactly equal {res.exact_share:.8f}, zero signs {res.zero_sign}, smallest |x| over 1 ulp {res.first_over_one!r}" if against == "f64" else "")
              + f", {res.seconds:.1f} s", flush=True)
        if res.mismatches:
            print("   ", res.message(), flush=True)
    return res


if __name__ == "__main__":
    argv = sys.argv[1:]
    opt = {"--arm": "device", "--against": "oracle", "--stride": str(STRIDE)}
    for k in list(opt):
        if k in argv:
            i = argv.index(k)
            opt[k] = argv[i + 1]
            del argv[i:i + 2]
    mode = argv[0] if argv else "default"
    assert mode in ("default", "full"), __doc__
    names = argv[1:] or (api.MATH_HOST_FNS if opt["--arm"] == "host" else FUNCTIONS)
    failed = 0
    for nm in names:
        failed += run(nm, mode, opt["--arm"], opt["--against"], int(opt["--stride"]), verbose=True).mismatches != 0
    sys.exit(1 if failed and opt["--against"] == "oracle" else 0)
