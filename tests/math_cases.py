"""Arguments at which the restated libm (clrrt_glibc.hpp, clrrt_glibcf.hpp) changes path, for the fn codes of
clrrt_selftest_math: every branch threshold, every table-row boundary, the neighbours of the multiples of pi/2,
axes, signed zeros, subnormals, infinities and NaN, plus the operands on which only an IEEE-exact sqrt / division
/ denormal handling gives the right bits.  Plain numpy, deterministic, no GPU.

    edge_cases(fn) -> (a, b, in_domain)    the edge set of fn's family; in_domain marks the cases the
                                           restatement answers itself (the others go to the GPU math library)
    sweep(fn, n)   -> (a, b)               n log-uniform arguments over the restated domain (all in domain)
    golden_index(family)                   the cases tests/golden/math_edges.npz records: every threshold case,
                                           the table-boundary and filler lists thinned by a stride

The constants below are copied from clrrt_glibc_data.hpp / clrrt_glibc.hpp / clrrt_glibcf.hpp under their names
there; test_math_edges_host.py checks the copies against the headers' text.
"""
import functools
import os
from decimal import Decimal, getcontext

import numpy as np

getcontext().prec = 80
PI = Decimal("3.14159265358979323846264338327950288419716939937510582097494459230781640628620899")
LN2 = Decimal("0.69314718055994530941723212145817656807550013436025525412068000949339362196969472")

# ---- clrrt_glibc_data.hpp
big = float.fromhex("0x1.8000000000000p+45")
hp0 = float.fromhex("0x1.921fb54442d18p+0")
taylor_lim = float.fromhex("0x1.020c49ba5e354p-3")
tan_g1 = float.fromhex("0x1.b096c00000000p-27")
tan_g2 = float.fromhex("0x1.f212d00000000p-5")
tan_g3 = float.fromhex("0x1.92f1a00000000p-1")
two8 = float.fromhex("0x1p+8")
mfftnhf = float.fromhex("-0x1.f000000000000p+3")
SINCOSTAB_N = 440
XFG_ROWS = 186
ATAN2_CIJ_ROWS = 241
at_inv16 = float.fromhex("0x1p-4")
# ---- clrrt_glibc.hpp: the hi-word thresholds of sin / cos / sincos and their select forms
SIN_HI_THRESHOLDS = (0x3e400000, 0x3e500000, 0x3feb6000, 0x400368fd, 0x419921fb)
SIN_HI_END = 0x419921fb            # |x| with hi word >= this: outside the restated domain
SIN_DOMAIN_END = 105414350.0       # the header's statement of the same bound
# glibc::exp: top12 of 2^-54, 512, 1024; the overflow bound, the first subnormal result, the last non-zero result
EXP_TOP12 = (0x3c9, 0x408, 0x409)
EXP_OVERFLOW = float.fromhex("0x1.62e42fefa39efp+9")
EXP_SUBNORMAL = float.fromhex("-0x1.6232bdd7abcd2p+9")
EXP_ZERO = float.fromhex("-0x1.74910d52d3051p+9")
# glibc::sincosf: abstop12 compares of pi/4, 2^-12, 120 and inf, as float words (abstop12 << 20), and pi/4 itself
SINCOSF_WORDS = (0x3f400000, 0x39800000, 0x42f00000, 0x7f800000, 0x3f490fdb)
# clrrt_glibcf.hpp: the word thresholds of acosf, asinf, atanf
ACOSF_WORDS = (0x3f800000, 0x3f000000, 0x32800000)
ASINF_WORDS = (0x3f800000, 0x3f000000, 0x32000000, 0x3F79999A)
ATANF_WORDS = (0x4c000000, 0x7f800000, 0x3ee00000, 0x31000000, 0x3f980000, 0x3f300000, 0x401c0000)
# the special values of tests/native/atan2_check.cpp (sp[])
ATAN2_SP = (0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-310, -1e-310, 1e300, -1e300, 5e-324,
            2.2250738585072014e-308, 0.0625, 1e-160, 1e160)
FL_2PI = 6.283185307179586         # fl(2 pi), the divisor of the engine's fmod calls

FAMILY = {0: "sincos", 1: "sincos", 16: "sincos", 17: "sincos", 20: "sincos", 21: "sincos", 22: "sincos",
          23: "sincos", 2: "tan", 24: "step", 25: "step", 26: "step", 27: "step", 28: "step", 5: "atan2", 6: "exp",
          8: "float1", 9: "float1", 11: "float1", 12: "float1", 29: "float1", 10: "atan2f", 3: "sqrt", 13: "sqrtf",
          7: "div", 14: "fdiv", 4: "fmod", 15: "round"}
FNS = sorted(FAMILY)
FLOAT_FNS = {8, 9, 10, 11, 12, 13, 14, 29}
NAMES = {0: "sin", 1: "cos", 2: "tan", 3: "sqrt", 4: "fmod", 5: "atan2", 6: "exp", 7: "div", 8: "cosf", 9: "sinf",
         10: "atan2f", 11: "acosf", 12: "asinf", 13: "sqrtf", 14: "fdiv", 15: "round", 16: "sincos.sin",
         17: "sincos.cos", 20: "sincos_sel.sin", 21: "sincos_sel.cos", 22: "sin_cos_fma_sel.sin",
         23: "sin_cos_fma_sel.cos", 24: "step_trig.s2", 25: "step_trig.c2", 26: "step_trig.swp",
         27: "step_trig.cwp", 28: "step_trig.t3", 29: "atanf"}
MIN_IN_DOMAIN = 0.99


# ------------------------------------------------------------------------------------------------ helpers
def _d(x):
    return np.atleast_1d(np.asarray(x, dtype=np.float64))


def _from_words(hi, lo=0):
    return np.array((np.uint64(hi) << np.uint64(32)) | np.uint64(lo), dtype=np.uint64).view(np.float64)


def _ulps(x, ks):
    """x's neighbours k ulps away in magnitude, for every k of ks (x finite, its magnitude stays positive)."""
    x = _d(x)
    u = x.view(np.int64)
    sign, mag = u & np.int64(-2 ** 63), u & np.int64(2 ** 63 - 1)
    out = [(mag + np.int64(k)) | sign for k in ks if np.all(mag + np.int64(k) >= 0)]
    return np.concatenate(out).view(np.float64)


def _fwords(words):
    """float32 bit patterns as doubles."""
    with np.errstate(invalid="ignore"):  # signalling NaN patterns
        return np.asarray(words, dtype=np.uint32).view(np.float32).astype(np.float64)


def _fulps(words, ks):
    """The floats k patterns away from each word (both signs), as doubles."""
    w = np.asarray(words, dtype=np.int64)
    m = np.concatenate([w + k for k in ks])
    m = m[(m >= 0) & (m <= 0x7fffffff)]
    return _fwords(np.concatenate([m, m | 0x80000000]).astype(np.uint32))


def _f32(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def _both(x):
    x = _d(x)
    return np.concatenate([x, -x])


def _log_uniform(rng, n, e_lo, e_hi, signed=True):
    """n magnitudes 2^e (1 + f), e uniform in [e_lo, e_hi), f uniform in [0, 1); subnormal where e < -1022."""
    e = rng.integers(e_lo, e_hi, n)
    x = np.ldexp(1.0 + rng.random(n), e)
    x = np.where(x == 0.0, 5e-324, x)
    if signed:
        x = np.where(rng.random(n) < 0.5, -x, x)
    return x


def _nearest(dec):
    return float(dec)  # Decimal -> double is correctly rounded


class _Set:
    """Segments of cases; keep = the stride at which tests/golden/math_edges.npz thins the segment (1: all)."""

    def __init__(self):
        self.seg = []

    def add(self, name, a, b=None, keep=1):
        a = _d(a)
        b = np.zeros_like(a) if b is None else np.broadcast_to(_d(b), a.shape).copy()
        assert a.shape == b.shape, name
        self.seg.append((name, a, b, keep))

    def arrays(self):
        return np.concatenate([s[1] for s in self.seg]), np.concatenate([s[2] for s in self.seg])

    def golden_index(self):
        idx, at = [], 0
        for _, a, _, keep in self.seg:
            idx.append(at + np.arange(0, len(a), keep))
            at += len(a)
        return np.concatenate(idx)


# ------------------------------------------------------------------------- sin / cos / sincos, select forms
def _pio2_multiples():
    last = int(Decimal(float(_from_words(SIN_HI_END))) / (PI / 2))  # the last multiple inside the domain
    ns = set(range(1, 65)) | {int(round(v)) for v in np.geomspace(65, last, 2000)} | {last}
    return sorted(ns)


def _sincos_set():
    s, rng = _Set(), np.random.default_rng(0x51C05)
    thr = [_from_words(T + dh, lo) for T in SIN_HI_THRESHOLDS for dh in (-1, 0, 1) for lo in (0, 1, 0xffffffff)]
    s.add("hi-word thresholds", _both(thr))
    k9 = range(-4, 5)
    s.add("taylor_lim", _both(_ulps(taylor_lim, k9)))
    # reduced arguments next to taylor_lim: n pi/2 +- taylor_lim (cos's case B hp0 - |x| is n = 1)
    red = [_nearest(Decimal(n) * PI / 2 + sg * Decimal(taylor_lim)) for n in range(1, 65) for sg in (-1, 1)]
    s.add("taylor_lim reduced", _both(_ulps(red, k9)))
    # sincostab rows: big + |x| rounds to the next 1/128 at (k + 1/2)/128, ties to even
    rows = SINCOSTAB_N // 4
    bnd = (np.arange(rows) + 0.5) / 128.0
    assert bnd[-1] == float(_from_words(0x3feb6000))  # the table ends where case B begins
    s.add("sincostab rows", _both(_ulps(bnd, (-1, 0, 1))), keep=2)
    redb = [_nearest(Decimal(n) * PI / 2 + sg * Decimal(float(v))) for n in (1, 2, 3, 4) for sg in (-1, 1)
            for v in bnd if v < 0.79]
    s.add("sincostab rows reduced", _both(_ulps(redb, (-1, 0, 1))), keep=16)
    mult = [_nearest(Decimal(n) * PI / 2) for n in _pio2_multiples()]
    s.add("pi/2 multiples 1..64", _both(_ulps(mult[:64], (-2, -1, 0, 1, 2))), keep=4)
    s.add("pi/2 multiples", _both(_ulps(mult[64:], (-2, -1, 0, 1, 2))), keep=16)
    s.add("tiny", _both(_log_uniform(rng, 4096, -1074, -20, signed=False)), keep=32)
    s.add("zeros", [0.0, -0.0])
    end = _ulps(SIN_DOMAIN_END, (0, 1, 2))
    s.add("out of domain", np.concatenate([_both(end), [1e300, np.inf, -np.inf, np.nan]]))
    # what the GPU math library's own reduction is measured on (the out-of-domain distance of DESIGN.md section 5)
    s.add("out of domain, up to 2^1023", _log_uniform(rng, 192, 27, 1023), keep=8)
    return s


def _sin_domain(a):
    hi = (_d(a).view(np.uint64) >> np.uint64(32)).astype(np.uint32) & np.uint32(0x7fffffff)
    return hi < np.uint32(SIN_HI_END)


# ------------------------------------------------------------------------------------------------------ tan
def _tan_set():
    s, rng = _Set(), np.random.default_rng(0x7A4)
    s.add("g1 g2 g3", _both(_ulps([tan_g1, tan_g2, tan_g3], range(-4, 5))))
    # xfg rows: (int)fma(w, two8, mfftnhf) steps at w = (i - mfftnhf) / two8; rows below 0 are the clamped side
    i_lo, i_hi = int(tan_g2 * two8 + mfftnhf), int(tan_g3 * two8 + mfftnhf)
    assert (i_lo, i_hi) == (0, XFG_ROWS - 1)
    bnd = (np.arange(-15, XFG_ROWS + 1) - mfftnhf) / two8
    bnd = bnd[bnd <= tan_g3]
    s.add("xfg rows", _both(_ulps(bnd, (-1, 0, 1))), keep=4)
    s.add("zeros", [0.0, -0.0])
    s.add("subnormal", _both(_log_uniform(rng, 256, -1074, -1022, signed=False)), keep=16)
    s.add("below g1", _log_uniform(rng, 256, -1022, -27), keep=16)
    s.add("polynomial and table", np.concatenate([_log_uniform(rng, 512, -27, -1), rng.uniform(-tan_g3, tan_g3, 512)]),
          keep=16)
    s.add("out of domain", np.concatenate([_both([1.0, 1.5707963267948966, 10.0, 1e5]), [1e300, np.inf, -np.inf, np.nan]]))
    return s


def _tan_domain(x):
    return np.abs(_d(x)) <= tan_g3


# ------------------------------------------------------------------------------- step_trig (x2 = a, x3 = b)
def _step_set():
    s = _Set()
    sa, _ = _sincos_set().arrays()
    ta, _ = _tan_set().arrays()
    sin_in, sin_out = sa[_sin_domain(sa)], sa[~_sin_domain(sa)]
    tan_in, tan_out = ta[_tan_domain(ta)], ta[~_tan_domain(ta)]
    s.add("x2 edges", sin_in, np.resize(tan_in, len(sin_in)), keep=64)
    s.add("x3 edges", np.resize(sin_in[::7], len(tan_in)), tan_in, keep=16)
    # one argument outside the block's domain: the hook takes sincos_sel / sin_cos_fma_sel / tan instead
    s.add("x3 out of domain", np.resize(sin_in[::11], 8 * len(tan_out)), np.resize(tan_out, 8 * len(tan_out)))
    s.add("x2 out of domain", np.resize(sin_out, len(sin_out)), np.resize(tan_in[::5], len(sin_out)))
    return s


# ---------------------------------------------------------------------------------------------------- atan2
def _atan2_pairs():
    """(y, x, keep) segments; glibc::atan2(y, x) is fn 5 with a = y, b = x."""
    seg = []
    sp = np.array(ATAN2_SP)
    seg.append(("sp x sp", np.repeat(sp, len(sp)), np.tile(sp, len(sp)), 1))
    quad = [(1, 1), (1, -1), (-1, 1), (-1, -1)]

    def ratios(name, u, keep):
        # u = min / max of |x|, |y| next to a branch value: both orientations, four quadrants, the 2^+-500
        # rescaling on either side and a denominator that is no power of two
        uk = _ulps(u, (-2, -1, 0, 1, 2))
        ys, xs = [], []
        for scale in (1.0, 2.0 ** -600, 2.0 ** 600):
            ys += [uk * scale, np.full_like(uk, scale)]
            xs += [np.full_like(uk, scale), uk * scale]
        ys += [uk * 3.0, np.full_like(uk, 3.0)]
        xs += [np.full_like(uk, 3.0), uk * 3.0]
        y, x = np.concatenate(ys), np.concatenate(xs)
        seg.append((name, np.concatenate([sy * y for sy, _ in quad]), np.concatenate([sx * x for _, sx in quad]), keep))

    ratios("1/16 and 1", [at_inv16, 1.0], 1)
    # atan2_row: i = (int)((u * 256 + 2^52) - 2^52) steps at (j + 1/2) / 256, j = 16 .. 255 (rows 0 .. 240)
    assert 256 - 16 + 1 == ATAN2_CIJ_ROWS
    ratios("cij rows", (np.arange(16, 256) + 0.5) / 256.0, 64)
    rng = np.random.default_rng(0xA7A2)
    r = rng.uniform(0.01, 50.0, 256)
    seg.append(("y = +-x", np.concatenate([r, r, -r, -r]), np.concatenate([r, -r, r, -r]), 8))
    ang = np.concatenate([np.array([0.7853981633974483, -0.7853981633974483])[rng.integers(0, 2, 1024)]
                          + (rng.random(1024) - 0.5) * 1e-12])
    rad = 0.2 + rng.random(1024) * 40
    seg.append(("pi/4 +- 1e-12", rad * np.sin(ang), rad * np.cos(ang), 8))
    # exponent differences around the de cut-offs (57 binades) and quotients that overflow or underflow
    ey, ex = [], []
    for de in (55, 56, 57, 58, 1000, 1074, 2000):
        for m in (1.0, 1.5, 1.9999999999999998):
            ey += [np.ldexp(m, de // 2), np.ldexp(1.25, -(de - de // 2))]
            ex += [np.ldexp(1.25, -(de - de // 2)), np.ldexp(m, de // 2)]
    ey, ex = np.array(ey), np.array(ex)
    seg.append(("exponent gaps", np.concatenate([sy * ey for sy, _ in quad]), np.concatenate([sx * ex for _, sx in quad]), 1))
    return seg


def _atan2_set():
    s = _Set()
    for name, y, x, keep in _atan2_pairs():
        s.add(name, y, x, keep)
    return s


# ------------------------------------------------------------------------------------------------------ exp
def _exp_set():
    s, rng = _Set(), np.random.default_rng(0xE4B)
    tops = np.concatenate([_from_words(t << 20).reshape(1) for t in EXP_TOP12])
    s.add("top12 thresholds", _both(_ulps(tops, range(-2, 3))))
    s.add("overflow, subnormal, zero", _ulps([EXP_OVERFLOW, EXP_SUBNORMAL, EXP_ZERO], range(-4, 5)))
    s.add("specials", [0.0, -0.0, np.inf, -np.inf, np.nan, 1e300, -1e300, 5e-324, -5e-324, -1000.0, 1000.0])
    # x = k ln2/128 + r: the table index k mod 128 steps at (k + 1/2) ln2/128, and r cancels to ~0 at k ln2/128
    k_lo, k_hi = int(Decimal("-745.2") * 128 / LN2), int(Decimal("709.8") * 128 / LN2)
    ks = np.unique(np.linspace(k_lo, k_hi, 512).astype(np.int64))
    half = [_nearest((Decimal(int(k)) + Decimal("0.5")) * LN2 / 128) for k in ks]
    whole = [_nearest(Decimal(int(k)) * LN2 / 128) for k in ks if k != 0]
    s.add("index boundaries", _ulps(half, (-1, 0, 1)), keep=4)
    s.add("index grid points", _ulps(whole, (-1, 0, 1)), keep=4)
    # exp_specialcase's two sides, whose roundings differ from the main path's and from each other's
    s.add("specialcase", np.concatenate([rng.uniform(512.0, EXP_OVERFLOW, 4096), rng.uniform(EXP_ZERO, -512.0, 4096)]),
          keep=16)
    s.add("-W3 D",np.concatenate([np.linspace(-260.0, 0.0, 4097), rng.uniform(-260.0, 0.0, 8192)]), keep=32)
    return s


# ---------------------------------------------------------------------------------------------- float functions
def _float1_set():
    s, rng = _Set(), np.random.default_rng(0xF10A7)
    s.add("pattern sweep", _fwords(np.arange(1, 2 ** 32, 4099, dtype=np.uint64).astype(np.uint32)), keep=509)
    k5 = range(-2, 3)
    s.add("sincosf thresholds", _fulps(SINCOSF_WORDS, k5))
    s.add("acosf asinf thresholds", _fulps(ACOSF_WORDS + ASINF_WORDS, k5))
    s.add("atanf thresholds", _fulps(ATANF_WORDS, k5))
    s.add("zeros", [0.0, -0.0])
    sub = np.concatenate([np.arange(1, 257), 0x007fffff - np.arange(0, 64), rng.integers(1, 0x00800000, 512)])
    s.add("subnormal", _fwords(np.concatenate([sub, sub | 0x80000000]).astype(np.uint32)), keep=8)
    return s


def _atan2f_set():
    s, rng = _Set(), np.random.default_rng(0xA7A2F)
    for name, y, x, keep in _atan2_pairs():
        s.add(name, _f32(y), _f32(x), keep)  # (1e300, 1e160 become inf: more special pairs)
    quad = [(1, 1), (1, -1), (-1, 1), (-1, -1)]
    # k = exponent difference against +-60, and x = 1 (atanf called directly)
    ey = np.array([np.ldexp(m, e) for e in (58, 59, 60, 61, 62, -58, -59, -60, -61, -62) for m in (1.0, 1.5, 1.9999999)])
    ex = np.full_like(ey, 1.5)
    s.add("exponent gaps", np.concatenate([sy * ey for sy, _ in quad]), np.concatenate([sx * ex for _, sx in quad]))
    one = _fulps(ATANF_WORDS, range(-2, 3))
    s.add("x = 1", one, np.ones_like(one))
    # subnormal operands and subnormal quotients
    sub = _fwords(np.concatenate([np.arange(1, 129), rng.integers(1, 0x00800000, 384)]).astype(np.uint32))
    den = rng.uniform(0.5, 4.0, len(sub)).astype(np.float32).astype(np.float64)
    s.add("subnormal", np.concatenate([sub, -sub, den, den]), np.concatenate([den, -den, sub, -sub]), keep=8)
    small = np.ldexp(1.0 + rng.random(256), rng.integers(-100, -60, 256)).astype(np.float32).astype(np.float64)
    large = np.ldexp(1.0 + rng.random(256), rng.integers(40, 60, 256)).astype(np.float32).astype(np.float64)
    s.add("subnormal quotient", np.concatenate([small, -small]), np.concatenate([large, large]), keep=8)
    return s


# ---------------------------------------------------------------------------------------------- basic operations
def _sqrt_set():
    s, rng = _Set(), np.random.default_rng(0x5071)
    k = np.concatenate([np.arange(1, 513), 2 ** 26 + np.arange(-32, 33), [2 ** 26.5 // 1, 94906265, 94906266]]).astype(np.float64)
    s.add("perfect squares", _ulps(k * k, (-1, 0, 1)), keep=8)
    s.add("subnormal", np.concatenate([_log_uniform(rng, 256, -1074, -1022, signed=False),
                                       _d(np.arange(1, 17) * 5e-324), _ulps(2.2250738585072014e-308, range(-4, 5))]), keep=4)
    s.add("near max", _ulps(1.7976931348623157e308, range(-8, 1)))
    s.add("specials", [0.0, -0.0, np.inf, 1.0, 2.0, 4.0])
    s.add("ordinary", _log_uniform(rng, 2048, -1022, 1023, signed=False), keep=32)
    return s


def _sqrtf_set():
    s, rng = _Set(), np.random.default_rng(0x5072)
    k = np.concatenate([np.arange(1, 4097), [4095.0, 5792.0, 5793.0]]).astype(np.float32)
    sq = (k * k).view(np.uint32).astype(np.int64)
    s.add("perfect squares", _fwords(np.concatenate([sq - 1, sq, sq + 1]).astype(np.uint32)), keep=32)
    sub = np.concatenate([np.arange(1, 257), 0x007fffff - np.arange(0, 64), 0x00800000 + np.arange(0, 8),
                          rng.integers(1, 0x00800000, 1024)])
    s.add("subnormal", _fwords(sub.astype(np.uint32)), keep=8)
    s.add("near max", _fwords((0x7f7fffff - np.arange(0, 16)).astype(np.uint32)))
    s.add("specials", [0.0, -0.0, np.inf, 1.0, 2.0, 4.0])
    s.add("ordinary", _fwords(rng.integers(0x00800000, 0x7f800000, 4096).astype(np.uint32)), keep=32)
    return s


def _div_set():
    s, rng = _Set(), np.random.default_rng(0xD17)
    n = 1024
    num, den = _log_uniform(rng, n, -600, -480), _log_uniform(rng, n, 440, 560)
    s.add("subnormal quotient", num, den, keep=8)
    # ties exist only among subnormal quotients: an odd multiple of 2^-1074 halved, a normal with an odd last bit
    odd = np.arange(1, 256, 2) * 5e-324
    low = np.ldexp(1.0 + (2 * np.arange(64) + 1) * 2.0 ** -52, -1022)
    t = np.concatenate([odd, low, np.ldexp(1.0 + (2 * np.arange(64) + 1) * 2.0 ** -52, -1021)])
    s.add("ties", np.concatenate([t, -t, t]), np.concatenate([np.full_like(t, 2.0), np.full_like(t, 2.0), np.full_like(t, -4.0)]),
          keep=4)
    s.add("subnormal operands", _log_uniform(rng, 512, -1074, -1022), _log_uniform(rng, 512, -1074, -1022), keep=8)
    s.add("specials", [0.0, -0.0, 1.0, 1.0, np.inf, 1.7976931348623157e308, 5e-324], [1.0, 3.0, 3.0, 5e-324, 2.0, 0.5, 1.7976931348623157e308])
    s.add("ordinary", rng.uniform(-60, 60, 4096), rng.uniform(-60, 60, 4096), keep=32)
    return s


def _fdiv_set():
    s, rng = _Set(), np.random.default_rng(0xFD17)

    def f(x):
        return np.asarray(x, dtype=np.float32).astype(np.float64)

    n = 1024
    num = f(np.ldexp(1.0 + rng.random(n), rng.integers(-100, -60, n)) * np.where(rng.random(n) < 0.5, -1, 1))
    den = f(np.ldexp(1.0 + rng.random(n), rng.integers(30, 64, n)))
    s.add("subnormal quotient", num, den, keep=8)
    odd = _fwords(np.arange(1, 256, 2).astype(np.uint32))
    low = _fwords((0x00800001 + 2 * np.arange(64)).astype(np.uint32))
    t = np.concatenate([odd, low, 2.0 * low])
    s.add("ties", np.concatenate([t, -t, t]), np.concatenate([np.full_like(t, 2.0), np.full_like(t, 2.0), np.full_like(t, -4.0)]),
          keep=4)
    sub = _fwords(rng.integers(1, 0x00800000, 1024).astype(np.uint32))
    s.add("subnormal operands", sub[:512], sub[512:], keep=8)
    s.add("subnormal by ordinary", sub[:512], f(rng.uniform(0.5, 4.0, 512)), keep=8)
    s.add("specials", [0.0, -0.0, 1.0, 1.0, np.inf], [1.0, 3.0, 3.0, float(np.float32(1e-45)), 2.0])
    s.add("ordinary", f(rng.uniform(-60, 60, 4096)), f(rng.uniform(-60, 60, 4096)), keep=32)
    return s


def _fmod_set():
    s, rng = _Set(), np.random.default_rng(0xF30D)
    ks = np.unique(np.concatenate([np.arange(1, 65), np.geomspace(65, 1e6 / FL_2PI, 256).astype(np.int64)])).astype(np.float64)
    s.add("k fl(2 pi)", _both(_ulps(ks * FL_2PI, (-1, 0, 1))), keep=8)
    s.add("below 2 pi", np.concatenate([_both(_ulps(FL_2PI, (-2, -1, 0, 1, 2))), rng.uniform(-FL_2PI, FL_2PI, 512)]), keep=8)
    s.add("up to 1e6", np.concatenate([rng.uniform(-1e6, 1e6, 2048), -rng.uniform(0, 1e6, 1024)]), keep=32)
    s.add("zeros and tiny", np.concatenate([[0.0, -0.0, 5e-324, -5e-324], _log_uniform(rng, 64, -1074, -1000)]), keep=4)
    s2 = _Set()
    for name, x, _, keep in s.seg:
        s2.add(name, x, np.full_like(x, FL_2PI), keep)
    return s2


def _round_set():
    s, rng = _Set(), np.random.default_rng(0x40D)
    k = np.arange(-64, 65).astype(np.float64)
    s.add("k +- 0.5", np.concatenate([k - 0.5, k + 0.5, k]), keep=4)
    h = 0.49999999999999994
    s.add("below one half", _both(_ulps([h, 0.5, 1.5 - 2.0 ** -52, 2.5], (-1, 0, 1))))
    t52 = 2.0 ** 52
    s.add("2^52", _both(np.concatenate([_ulps([t52, t52 / 2, t52 / 4, 2 * t52], range(-4, 5))])))
    s.add("specials", [0.0, -0.0, np.inf, -np.inf, 1e300, -1e300, 5e-324, -5e-324])
    s.add("ordinary", rng.uniform(-500, 500, 1024), keep=16)
    return s


_BUILDERS = {"sincos": _sincos_set, "tan": _tan_set, "step": _step_set, "atan2": _atan2_set, "exp": _exp_set,
             "float1": _float1_set, "atan2f": _atan2f_set, "sqrt": _sqrt_set, "sqrtf": _sqrtf_set, "div": _div_set,
             "fdiv": _fdiv_set, "fmod": _fmod_set, "round": _round_set}
FAMILIES = sorted(_BUILDERS)


@functools.lru_cache(maxsize=None)
def _family(name):
    s = _BUILDERS[name]()
    a, b = s.arrays()
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b, s.golden_index(), [(n, len(x)) for n, x, _, _ in s.seg]


def in_domain(fn, a, b):
    """Where the restatement answers fn itself (elsewhere it hands the call to the GPU math library)."""
    fam = FAMILY[fn]
    if fam == "sincos" or fn in (24, 25, 26, 27):
        return _sin_domain(a)
    if fam == "tan":
        return _tan_domain(a)
    if fn == 28:
        return _tan_domain(b)
    return np.ones(len(a), dtype=bool)  # total functions: NaN, inf and every finite argument are restated


def family_cases(name):
    a, b, _, _ = _family(name)
    return a, b


def golden_index(name):
    return _family(name)[2]


def segments(name):
    return _family(name)[3]


def edge_cases(fn):
    a, b = family_cases(FAMILY[fn])
    dom = in_domain(fn, a, b)
    # a later edit cannot empty the bit-exact check by re-flagging cases
    assert dom.mean() >= MIN_IN_DOMAIN, (NAMES[fn], float(dom.mean()))
    return a, b, dom


# ----------------------------------------------------------------------------------------------------- sweeps


@functools.lru_cache(maxsize=None)
def _family_sweep(name, n):
    rng = np.random.default_rng([0x5EE9, FAMILIES.index(name)])
    zero = np.zeros(n)
    if name == "sincos":
        a = _log_uniform(rng, n, -40, 27)
        a = np.where(_sin_domain(a), a, a * 0.5)  # the top binade ends at the domain's end
        b = zero
    elif name == "tan":
        a = _log_uniform(rng, n, -40, 0)
        a, b = np.where(_tan_domain(a), a, a * 0.5), zero
    elif name == "step":
        a, _ = _family_sweep("sincos", n)
        b, _ = _family_sweep("tan", n)
        b = b[::-1].copy()
    elif name == "atan2":
        a, b = _log_uniform(rng, n, -30, 30), _log_uniform(rng, n, -30, 30)
        near = rng.random(n) < 0.5  # |y / x| within a factor 32 of 1: the table rows
        b = np.where(near, a * np.ldexp(1.0 + rng.random(n), rng.integers(-5, 5, n)) * np.where(rng.random(n) < 0.5, -1, 1), b)
    elif name == "exp":
        a, b = _log_uniform(rng, n, -60, 10), zero
        a = np.where(np.abs(a) > 746.0, a * 0.5, a)
    elif name == "float1":
        a, b = _f32(_log_uniform(rng, n, -32, 30)), zero
    elif name == "atan2f":
        a, b = _f32(_log_uniform(rng, n, -30, 30)), _f32(_log_uniform(rng, n, -30, 30))
    elif name == "sqrt":
        a, b = _log_uniform(rng, n, -1074, 1024, signed=False), zero
    elif name == "sqrtf":
        a, b = _f32(_log_uniform(rng, n, -126, 128, signed=False)), zero
    elif name == "div":
        a, b = _log_uniform(rng, n, -540, 540), _log_uniform(rng, n, -540, 540)
    elif name == "fdiv":
        a, b = _f32(_log_uniform(rng, n, -75, 75)), _f32(_log_uniform(rng, n, -75, 75))
    elif name == "fmod":
        a, b = _log_uniform(rng, n, -10, 20), np.full(n, FL_2PI)
    elif name == "round":
        a, b = _log_uniform(rng, n, -3, 54), zero
    else:
        raise KeyError(name)
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def sweep(fn, n=1 << 20):
    a, b = _family_sweep(FAMILY[fn], n)
    if fn in (11, 12):  # acosf / asinf: |x| <= 1, log-uniform towards 0
        a = _f32(np.where(np.abs(a) > 1.0, 1.0 / a, a))
    assert in_domain(fn, a, b).all(), NAMES[fn]
    return a, b


# ------------------------------------------------------------------------- tests/golden/math_edges.npz
# libm gives the select forms the values of the functions they restate: one record serves each group
GOLDEN_FN = {20: 16, 21: 17, 22: 0, 23: 1}
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "math_edges.npz")


def golden_key(fn):
    return f"{FAMILY[fn]}.{NAMES[GOLDEN_FN.get(fn, fn)]}"


def golden_pack(fn, values):
    """The recorded form of libm's values: the bits of the double, or of the float for the float functions."""
    values = np.asarray(values, dtype=np.float64)
    return _f32(values).astype(np.float32).view(np.uint32) if fn in FLOAT_FNS else values.view(np.uint64)


def golden_unpack(fn, rec):
    return rec.view(np.float32).astype(np.float64) if fn in FLOAT_FNS else rec.view(np.float64)


def golden_cases(fn, z):
    """(a, b, libm's recorded values) of fn from the loaded file z."""
    fam = FAMILY[fn]
    a = z[f"{fam}.a"].view(np.float64)
    b = z[f"{fam}.b"].view(np.float64) if f"{fam}.b" in z else np.zeros_like(a)
    return a, b, golden_unpack(fn, z[golden_key(fn)])
