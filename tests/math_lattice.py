"""Chosen operands for every expression operator (hnb_math.h, hnb_vm.h) and an independent reference of what each must give.

Data and numpy only: no oracle, no hnb_math.h. The operands sit on the seams where a device compile, a hiprtc compile and the host
compile of the same header can part ways: the |x| = 65536 switch of the trigonometric reduction and arguments next to k pi/2, the
|x| = 1/2 switch of asin / acos, the tan(pi/8) / tan(3 pi/8) switches of atan, the mantissa seam of f_log_reduce, subnormal arguments
and results, the saturation clamps of exp / exp2 / pow, correctly rounded division and sqrt on subnormals, float <-> int saturation,
INT_MIN / -1. Every float group carries COMMON (the zeros, four subnormal landmarks, the largest finite value, the infinities, NaN).

The reference:
  * transcendental functions: numpy's binary64 libm rounded once to binary32 (`ref_unary`, `ref_pow`, `ref_atan2`);
  * + - * / sqrt floor ceil round-even: numpy binary32 arithmetic, which is exact IEEE-754 (one rounding per operation);
  * everything else: the WGSL formula written out in numpy, one binary32 operation per step.
PINNED lists the operands where the project's definition departs from libm, each with the value it is pinned to: a test asserts
those instead of leaving them out (`apply_pins`).

Everything is deterministic: no random numbers but the fixed-seed pow leg of tests/test_math.py.
"""
import numpy as np

f32, f64, u32, i32 = np.float32, np.float64, np.uint32, np.int32
INF, NAN = f32(np.inf), f32(np.nan)
FLT_MAX = f32(3.4028234663852886e38)


# ---- stepping through the binary32 number line -----------------------------------------------------------------------------------
def _ordered(x):
    """binary32 -> int64 that increases with the value (-0 and +0 both map to 0)"""
    b = np.asarray(x, f32).view(i32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def _from_ordered(o):
    o = np.asarray(o, np.int64)
    return np.where(o < 0, (-o) | 0x80000000, o).astype(u32).view(f32)


def step_ulps(x, n):
    """the float n places up (n < 0: down) the number line from x"""
    return _from_ordered(_ordered(x) + n)


def around(x, n):
    """x with its n neighbours on each side"""
    x = np.atleast_1d(np.asarray(x, f32))
    return np.concatenate([step_ulps(x, k) for k in range(-n, n + 1)]).astype(f32)


def ulp_diff(a, b):
    return np.abs(_ordered(a) - _ordered(b))


def cat(*parts):
    return np.concatenate([np.atleast_1d(np.asarray(p, f64)).astype(f32) for p in parts])


def cross(a, b):
    """every pair (a_i, b_j) as two flat arrays"""
    aa, bb = np.meshgrid(np.asarray(a), np.asarray(b), indexing="ij")
    return aa.ravel().copy(), bb.ravel().copy()


def cross3(a, b, c):
    aa, bb, cc = np.meshgrid(np.asarray(a), np.asarray(b), np.asarray(c), indexing="ij")
    return aa.ravel().copy(), bb.ravel().copy(), cc.ravel().copy()


SUBNORMAL = cat(2.0 ** -149, 2.0 ** -127, step_ulps(f32(2.0 ** -126), -1), 2.0 ** -126)   # smallest, a middle one, the largest, the first normal
COMMON = cat(0.0, -0.0, SUBNORMAL, FLT_MAX, np.inf, -np.inf, np.nan)
COMMON_SIGNED = cat(COMMON, -SUBNORMAL, -FLT_MAX)

TAN_PIO8, TAN_3PIO8 = f32(float.fromhex("0x1.a8279ap-2")), f32(float.fromhex("0x1.3504f4p+1"))
TWO40 = f32(2.0 ** 40)

# the landmark set of the IEEE operators; its cross product has quotients that round into the subnormals (2^-100 / 2^64, 1/3 * 2^-126 ...)
# and quotients and products one ulp below overflow (prev(max) / prev(1) ...)
_LAND_POS = cat(SUBNORMAL, 1.0, step_ulps(f32(1.0), -1), step_ulps(f32(1.0), 1), 3.0, 1.0 / 3.0, 2.0, 0.5, 1.5, 2.5, 2.0 ** 64, 2.0 ** -64, 2.0 ** 100, 2.0 ** -100,
                1e30, 1e-30, TAN_PIO8, TAN_3PIO8, around(FLT_MAX, 2)[:3], 2.0 ** 23 + 1.0, 2.0 ** 24, 0.49999997)
LANDMARKS = cat(0.0, -0.0, _LAND_POS, -_LAND_POS, np.inf, -np.inf, np.nan)
# a smaller set for the three-operand operators
LANDMARKS3 = cat(0.0, -0.0, 2.0 ** -149, -(2.0 ** -126), 0.25, 0.5, 1.0, -1.0, 1.0 / 3.0, 3.0, -2.5, 1e30, FLT_MAX, -FLT_MAX, np.inf, -np.inf, np.nan)
MIX_T = cat(0.0, 1.0, np.nan, np.inf)
# both operands of the operators evaluated in the uniform stream (one frame per pair)
UNIFORM_SET = cat(COMMON, -(2.0 ** -149), 1.0, -1.0, 0.5, step_ulps(f32(0.5), 1), 1.0 / 3.0, 3.0, 65536.0, step_ulps(f32(65536.0), 1), 2.0 ** 40, 2.0 ** -64, 1e30, 88.7228, -103.972,
                  TAN_PIO8, u32(0x3F2AAAAB).view(f32), 2.5)


# ---- operands: one array per function family -------------------------------------------------------------------------------------
def trig_args():
    k = np.arange(1, 41722, dtype=f64)                                    # k pi/2 <= 65536
    near = (k * (np.pi / 2)).astype(f32)
    near = np.concatenate([step_ulps(near, -1), near, step_ulps(near, 1)])
    kb = np.round(np.geomspace(41723.0, 2.0 ** 40 / (np.pi / 2) - 2.0, 20000))    # 65536 < k pi/2 < 2^40: the binary64 reduction
    big = (kb * (np.pi / 2)).astype(f32)
    return cat(COMMON_SIGNED, near, -near, around(f32(65536.0), 3), -around(f32(65536.0), 3), big, -big[::16], around(TWO40, 3), -around(TWO40, 3),
               1e10, -1e10, 3.4e38, -3.4e38, 1e4, 12345.678, 1e6, 3.4e7, -7.7e6, 1e-30)


def atan_args():
    sw = cat(around(TAN_PIO8, 3), around(TAN_3PIO8, 3))
    t = np.tan(np.linspace(-np.pi / 2, np.pi / 2, 4003)[1:-1])
    return cat(COMMON_SIGNED, sw, -sw, 1.0, -1.0, 1e10, -1e10, 1e-10, -1e-10, t)


def unit_args():
    sw = cat(around(f32(0.5), 3), around(f32(1.0), 3))
    return cat(COMMON_SIGNED, sw, -sw, 2.0 ** -12, -(2.0 ** -12), np.sqrt(0.5), -np.sqrt(0.5), np.linspace(-1.0, 1.0, 4001))


def exp_args():
    k = np.arange(-151, 130, dtype=f64)
    return cat(COMMON_SIGNED, around(f32(88.7228), 4), around(f32(-87.3365), 4), around(f32(-103.972), 4), around(f32(90.0), 2), around(f32(-105.0), 2),
               k * np.log(2.0), (k + 0.5) * np.log(2.0), np.linspace(-104.0, -87.0, 3001), 1000.0, -1000.0, 1e30, -1e30)


def exp2_args():
    return cat(COMMON_SIGNED, np.arange(-152.0, 130.25, 0.5), around(f32(-126.0), 3), around(f32(-149.0), 3), around(f32(-149.5), 3), around(f32(-150.0), 3),
               around(f32(128.0), 3), around(f32(130.0), 2), around(f32(-152.0), 2), np.linspace(-150.0, -125.0, 5001), 1e30, -1e30)


def log_args():
    sub = np.arange(1, 4097, dtype=u32).view(f32)
    e = np.arange(-149, 128, dtype=f64)
    four3 = (f32(4.0 / 3.0).astype(f64) * 2.0 ** np.arange(-126, 127, dtype=f64))
    seams = cat(around(u32(0x3F2AAAAB).view(f32), 3), around(u32(0x3FAAAAAB).view(f32), 3))
    return cat(COMMON_SIGNED, sub, 2.0 ** e, four3, seams, around(f32(1.0), 4), 1.0 + 2.0 ** -12, 1.0 - 2.0 ** -12, np.linspace(0.6, 1.4, 8001), -1.0, _LAND_POS)


def landmark_pairs():
    return cross(LANDMARKS, LANDMARKS)


def landmark_triples():
    a, b, c = cross3(LANDMARKS3, LANDMARKS3, LANDMARKS3)
    ma, mb, mt = cross3(LANDMARKS3, LANDMARKS3, MIX_T)                       # mix with t in {0, 1, NaN, inf}: the third operand
    return np.concatenate([a, ma]), np.concatenate([b, mb]), np.concatenate([c, mt])


def rounding_args():
    """floor / ceil / round / fract / sign / saturate / abs: the landmarks and the ties of round-to-even"""
    h = np.arange(-4.5, 5.0, 0.5)
    big = cat(2.0 ** 22 + 0.5, 2.0 ** 23 - 0.5, 2.0 ** 23 + 1.0, 2.0 ** 31, -(2.0 ** 31))
    return cat(LANDMARKS, h, around(f32(0.5), 1), around(f32(-0.5), 1), around(f32(1.0), 1), big, -big)


POW_X = cat(0.0, -0.0, 1.0, step_ulps(f32(1.0), -1), step_ulps(f32(1.0), 1), 2.0, 0.5, 10.0, 1e30, 1e-30, 2.0 ** -149, FLT_MAX, np.inf, -1.0, np.nan)
POW_Y = cat(0.0, -0.0, 1.0, -1.0, 0.5, 1.0 / 3.0, 2.0, -2.0, 127.0, 128.0, -149.0, -150.0, 1e7, -1e7, 1e30, -1e30, np.inf, -np.inf, 2.0 ** -149, np.nan)


def pow_args():
    """the special-value cross product, then the sampled leg of tests/test_math.py (x in e^[-10, 10], y in [-8, 8])"""
    x, y = cross(POW_X, POW_Y)
    rng = np.random.default_rng(1234)
    return np.concatenate([x, np.exp(rng.uniform(-10, 10, 4000)).astype(f32)]), np.concatenate([y, rng.uniform(-8, 8, 4000).astype(f32)])


ATAN2_SET = cat(0.0, -0.0, 1.0, -1.0, 2.0 ** -149, -(2.0 ** -149), FLT_MAX, -FLT_MAX, np.inf, -np.inf, 1e30, 1e-30, TAN_PIO8, TAN_3PIO8)

F2I = cat(COMMON_SIGNED, around(f32(2.0 ** 31), 2), around(f32(-(2.0 ** 31)), 2), around(f32(2.0 ** 32), 2), 2.0 ** 31 - 128, -0.5, 0.5, 0.99999994, -0.99999994, 1.0, -1.0, 1.5,
          -1.5, 2.5, 16777216.0, 16777217.0, 123456.789, -123456.789, 4294967040.0, 3e9, -3e9, 1e10, -1e10)
I2F = np.array([0, 1, 2, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 2, (1 << 24) + 3, (1 << 25) + 2, (1 << 25) + 6, 0x7FFFFF80, 0x7FFFFFBF, 0x7FFFFFC0, 0x7FFFFFFF,
                0x80000000, 0x80000001, 0x80000080, 0x800000C0, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFE, 0xFFFFFFFF, 0xFF000001, 0xFEFFFFFF], dtype=u32)

INTS = np.array([0, 1, 2, 3, 7, 0x7FFFFFFE, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFF9, 0x0000FFFF, 0x00010000, 0x12345678, 0xCAFEF00D], dtype=u32)


def int_triples():
    return cross3(INTS, INTS, INTS[[0, 1, 6, 7, 8, 10]])


def pack_vectors():
    """vec4 operands of pack4x8unorm / pack4x8snorm: every combination is one component against fixed neighbours"""
    ks = np.array([0, 1, 2, 63, 127, 128, 254, 255], f64)
    c = cat(0.0, -0.0, np.nan, np.inf, -np.inf, FLT_MAX, -FLT_MAX, 2.0 ** -149, around(f32(1.0), 1), around(f32(-1.0), 1), around((ks / 255.0).astype(f32), 1),
            around(((ks + 0.5) / 255.0).astype(f32), 1), around((ks[:5] / 127.0).astype(f32), 1), -around((ks[:5] / 127.0).astype(f32), 1),
            around(((ks[:5] + 0.5) / 127.0).astype(f32), 1), -around(((ks[:5] + 0.5) / 127.0).astype(f32), 1))
    n = len(c)
    return np.stack([c, np.roll(c, 1), np.roll(c, n // 3), c[::-1]], axis=1).astype(f32)


def unpack_words():
    """every byte value in every lane"""
    b = np.arange(256, dtype=u32)
    return (b | (((b + 85) & 255) << 8) | (((b * 7 + 3) & 255) << 16) | ((255 - b) << 24)).astype(u32)


def vec3_pairs():
    """(a, b) vec3 operands of dot / cross / distance, a also of length / normalize: the tiny vectors of
    tests/test_math.py::test_normalize_reciprocal_domain, one whose squared length overflows, the zero vector, ordinary ones"""
    rows = []
    for e in (-149, -140, -126, -100, -75, -74, -70, -64):
        t = 2.0 ** e
        rows += [(t, 0, 0), (t, t, t), (t, -t, 0.5 * t)]
    rows += [(0, 0, 0), (-0.0, 0.0, -0.0), (2e19, 2e19, -2e19), (3e38, 1.0, 0.0), (1.0, 2.0, 3.0), (-0.3, 0.1, 7.5), (1.0 / 3.0, -2.0 / 3.0, 1e-3),
             (np.nan, 1.0, 0.0), (np.inf, 1.0, 0.0), (1e-20, 1e20, 1.0)]
    a = np.array(rows, f64).astype(f32)
    ia, ib = cross(np.arange(len(a)), np.arange(len(a)))
    return a[ia], a[ib]


# ---- the reference ---------------------------------------------------------------------------------------------------------------
_QUIET = dict(all="ignore")


def _narrow(x64):
    with np.errstate(**_QUIET):
        return np.asarray(x64, f64).astype(f32)


UNARY64 = {"sin": np.sin, "cos": np.cos, "tan": np.tan, "atan": np.arctan, "asin": np.arcsin, "acos": np.arccos, "exp": np.exp, "exp2": np.exp2,
           "log": np.log, "log2": np.log2}
# the ulp bounds of hanabi-math v3 against the correctly rounded result (tests/test_math.py MAX_ULP; every other function 1)
MAX_ULP = {"sin": 2, "cos": 2, "tan": 4, "asin": 2, "atan": 2, "atan2": 2, "pow": 8}
POW_MODERATE_ULP = 2            # pow where |y log2 x| <= 32


def ref_unary(name, x):
    with np.errstate(**_QUIET):
        return _narrow(UNARY64[name](np.asarray(x, f32).astype(f64)))


def ref_pow(x, y):
    with np.errstate(**_QUIET):
        return _narrow(np.power(np.asarray(x, f32).astype(f64), np.asarray(y, f32).astype(f64)))


def ref_atan2(y, x):
    with np.errstate(**_QUIET):
        return _narrow(np.arctan2(np.asarray(y, f32).astype(f64), np.asarray(x, f32).astype(f64)))


def pow_is_moderate(x, y):
    with np.errstate(**_QUIET):
        return np.abs(np.asarray(y, f64) * np.log2(np.asarray(x, f64))) <= 32.0


def _f(x):
    return np.asarray(x, f32)


def ref_min(a, b):
    return np.where(_f(b) < _f(a), b, a).astype(f32)          # WGSL: e2 < e1 ? e2 : e1


def ref_max(a, b):
    return np.where(_f(a) < _f(b), b, a).astype(f32)          # WGSL: e1 < e2 ? e2 : e1


def ref_clamp(x, lo, hi):
    return ref_min(ref_max(x, lo), hi)


def ref_ieee(name, a, b=None, c=None):
    """binary32 arithmetic, one rounding per step"""
    a = _f(a)
    b = None if b is None else _f(b)
    c = None if c is None else _f(c)
    one, zero = f32(1.0), f32(0.0)
    with np.errstate(**_QUIET):
        if name == "add": return a + b
        if name == "sub": return a - b
        if name == "mul": return a * b
        if name == "div": return a / b
        if name == "rem": return a - b * np.trunc(a / b)                      # WGSL: truncated remainder, the sign of the dividend
        if name == "min": return ref_min(a, b)
        if name == "max": return ref_max(a, b)
        if name == "step": return np.where(a <= b, one, zero).astype(f32)     # step(edge = a, x = b)
        if name == "sqrt": return np.sqrt(a)
        if name == "inverseSqrt": return one / np.sqrt(a)                     # two roundings
        if name == "floor": return np.floor(a)
        if name == "ceil": return np.ceil(a)
        if name == "round": return np.rint(a)                                 # ties to even
        if name == "fract": return a - np.floor(a)
        if name == "abs": return np.abs(a)
        if name == "sign": return np.where(a > zero, one, np.where(a < zero, -one, zero)).astype(f32)
        if name == "saturate": return ref_clamp(a, np.zeros_like(a), np.ones_like(a))
        if name == "clamp": return ref_clamp(a, b, c)
        if name == "mix": return a * (one - c) + b * c                        # mix(a, b, t = c)
        if name == "smoothstep":                                              # smoothstep(lo = a, hi = b, x = c)
            t = ref_clamp((c - a) / (b - a), np.zeros_like(a), np.ones_like(a))
            return t * t * (f32(3.0) - f32(2.0) * t)
    raise KeyError(name)


def ref_f2i(x):
    x = _f(x).astype(f64)
    with np.errstate(**_QUIET):
        t = np.clip(np.trunc(np.where(np.isnan(x), 0.0, x)), -2147483648.0, 2147483647.0)
    return t.astype(np.int64).astype(i32).view(u32)


def ref_f2u(x):
    x = _f(x).astype(f64)
    with np.errstate(**_QUIET):
        t = np.clip(np.trunc(np.where(np.isnan(x), 0.0, x)), 0.0, 4294967295.0)
    return t.astype(np.int64).astype(u32)


def ref_i2f(w):
    return np.asarray(w, u32).view(i32).astype(f32)       # round to nearest, ties to even


def ref_u2f(w):
    return np.asarray(w, u32).astype(f32)


def _trunc_div(a, b):
    """C's division on int64 operands (numpy's // floors), b != 0"""
    q = np.abs(a) // np.abs(b)
    return np.where((a < 0) != (b < 0), -q, q)


def ref_int(name, x, y=None, z=None, signed=True):
    """WGSL integer operators on u32 words; signed: the words are i32. x / 0 = x, x % 0 = 0, INT_MIN / -1 = INT_MIN, INT_MIN % -1 = 0."""
    view = (lambda w: np.asarray(w, u32).view(i32).astype(np.int64)) if signed else (lambda w: np.asarray(w, u32).astype(np.int64))
    a = view(x)
    b = None if y is None else view(y)
    c = None if z is None else view(z)
    wrap = lambda v: (np.asarray(v, np.int64) & 0xFFFFFFFF).astype(u32)
    if name in ("div", "rem"):
        safe = np.where(b == 0, 1, b)
        q = np.where(b == 0, a, _trunc_div(a, safe))           # (INT_MIN / -1 = 2^31 wraps to INT_MIN by itself)
        return wrap(q) if name == "div" else wrap(np.where(b == 0, 0, a - _trunc_div(a, safe) * safe))
    if name == "add": return wrap(a + b)
    if name == "sub": return wrap(a - b)
    if name == "mul": return wrap(a * b)
    if name == "min": return wrap(np.where(b < a, b, a))
    if name == "max": return wrap(np.where(a < b, b, a))
    if name == "clamp": return wrap(np.minimum(np.maximum(a, b), c))
    if name == "abs": return wrap(np.abs(a))                  # abs(INT_MIN) = INT_MIN
    if name == "sign": return wrap(np.sign(a))
    if name == "cmp": return ((a < b) * 1 + (a <= b) * 2 + (a > b) * 4 + (a >= b) * 8).astype(u32)
    raise KeyError(name)


def ref_pack(v, snorm):
    v = _f(v)
    with np.errstate(**_QUIET):
        if snorm:
            c = ref_min(np.ones_like(v), ref_max(-np.ones_like(v), v))        # min(1, max(-1, c)) in WGSL's definition of min / max: NaN -> -1
            w = np.floor(f32(0.5) + f32(127.0) * c).astype(np.int64) & 0xFF
        else:
            c = ref_min(np.ones_like(v), ref_max(np.zeros_like(v), v))        # NaN -> 0
            w = np.floor(f32(0.5) + f32(255.0) * c).astype(np.int64) & 0xFF
    return (w[:, 0] | (w[:, 1] << 8) | (w[:, 2] << 16) | (w[:, 3] << 24)).astype(u32)


def ref_unpack(w, snorm):
    w = np.asarray(w, u32)
    b = np.stack([(w >> s) & 0xFF for s in (0, 8, 16, 24)], axis=1)
    if snorm:
        return np.maximum(b.astype(np.uint8).view(np.int8).astype(f32) / f32(127.0), f32(-1.0)).astype(f32)
    return (b.astype(f32) / f32(255.0)).astype(f32)


def ref_vec3(name, a, b=None):
    """binary32, left to right: dot = (x x' + y y') + z z'; normalize(v) = v * (1 / length(v))"""
    a = _f(a)
    b = None if b is None else _f(b)
    sq = lambda v: (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    with np.errstate(**_QUIET):
        if name == "dot": return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
        if name == "length": return np.sqrt(sq(a))
        if name == "distance": return np.sqrt(sq(a - b))
        if name == "normalize": return a * (f32(1.0) / np.sqrt(sq(a)))[:, None]
        if name == "cross":
            return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
    raise KeyError(name)


# ---- where the project's definition is not libm's ---------------------------------------------------------------------------------
def _is_neg_zero(x):
    return _f(x).view(u32) == 0x80000000


def _no_nan(*xs):
    m = np.ones(np.shape(xs[0]), bool)
    for x in xs:
        m &= ~np.isnan(x)
    return m


# (function, what, mask over the operands, pinned value). The masks of one function do not overlap.
PINNED = [
    ("sin", "|x| > 2^40 is x = 0", lambda x: (np.abs(x) > TWO40) & np.isfinite(x), f32(0.0)),
    ("cos", "|x| > 2^40 is x = 0", lambda x: (np.abs(x) > TWO40) & np.isfinite(x), f32(1.0)),
    ("tan", "|x| > 2^40 is x = 0", lambda x: (np.abs(x) > TWO40) & np.isfinite(x), f32(0.0)),
    ("sin", "sin(-0) = +0", _is_neg_zero, f32(0.0)),
    ("tan", "tan(-0) = +0", _is_neg_zero, f32(0.0)),
    ("atan2", "atan2(+-inf, +-inf) = NaN", lambda y, x: np.isinf(y) & np.isinf(x), NAN),
    ("pow", "a NaN operand gives NaN (pow(NaN, 0), pow(1, NaN))", lambda x, y: np.isnan(x) | np.isnan(y), NAN),
    ("pow", "pow(x < 0, y != 0) = NaN", lambda x, y: _no_nan(x, y) & (x < 0) & (y != 0), NAN),
    ("pow", "pow(+-0, y < 0) = +inf", lambda x, y: (x == 0) & (y < 0), INF),
    ("pow", "pow(-0, y > 0) = +0", lambda x, y: _is_neg_zero(x) & (y > 0), f32(0.0)),
    ("pow", "pow(1, +-inf) = NaN", lambda x, y: (x == 1) & np.isinf(y), NAN),
]


def apply_pins(name, want, *operands):
    """`want` with the pinned values written over the reference's; also the mask of the pinned points"""
    want = np.array(want, f32)
    pinned = np.zeros(want.shape, bool)
    for fn, _, mask, value in PINNED:
        if fn == name:
            with np.errstate(**_QUIET):
                m = mask(*[_f(o) for o in operands])
            assert not (m & pinned).any(), (name, "two pins claim one operand")
            want[m] = value
            pinned |= m
    return want, pinned


# ---- comparisons -----------------------------------------------------------------------------------------------------------------
def float_class(x):
    """0 finite, 1 +inf, 2 -inf, 3 NaN"""
    x = _f(x)
    return np.where(np.isnan(x), 3, np.where(x == INF, 1, np.where(x == -INF, 2, 0)))


def same_bits(got, want):
    """elementwise: equal as uint32, or NaN on both sides (WGSL leaves the payload open, and two compilers do differ in it)"""
    got, want = _f(got), _f(want)
    return (got.view(u32) == want.view(u32)) | (np.isnan(got) & np.isnan(want))


def check_bits(what, got, want, *operands):
    ok = same_bits(got, want)
    if not ok.all():
        i = int(np.flatnonzero(~ok.reshape(len(ok), -1).all(axis=1))[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} results differ; first at operands {[np.asarray(o)[i] for o in operands]!r}: "
                             f"got {np.asarray(got)[i]!r} want {np.asarray(want)[i]!r}")


def check_words(what, got, want, *operands):
    got, want = np.asarray(got, u32).reshape(-1), np.asarray(want, u32).reshape(-1)
    bad = np.flatnonzero(got != want)
    if len(bad):
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} results differ; first at operands {[hex(int(np.asarray(o, u32).reshape(-1)[i])) for o in operands]}: "
                             f"got {int(got[i]):#x} want {int(want[i]):#x}")


def check_against_libm(name, got, want, pinned, operands, bound=None, moderate=None):
    """The assertions of one transcendental function over its lattice: the pinned points by bits, the NaN / inf / finite class at every
    point, the sign of every zero, every finite point within the function's ulp bound. Returns the worst distance seen."""
    got, want = _f(got), _f(want)
    where = lambda m: [np.asarray(o)[m][0] for o in operands]
    if pinned.any():
        ok = same_bits(got[pinned], want[pinned])
        assert ok.all(), f"{name}: pinned value missed at {[np.asarray(o)[pinned][~ok][0] for o in operands]!r}: got {got[pinned][~ok][0]!r} want {want[pinned][~ok][0]!r}"
    cls = float_class(got) != float_class(want)
    assert not cls.any(), f"{name}: {int(cls.sum())} results of another class (NaN / inf / finite); first at {where(cls)!r}: got {got[cls][0]!r} want {want[cls][0]!r}"
    zs = (want == 0) & (np.signbit(got) != np.signbit(want))
    assert not zs.any(), f"{name}: sign of zero differs at {where(zs)!r}"
    fin = np.isfinite(want) & ~pinned
    d = ulp_diff(got[fin], want[fin])
    bound = MAX_ULP.get(name, 1) if bound is None else bound
    if d.size:
        assert d.max() <= bound, f"{name}: {int(d.max())} ulp (bound {bound}) at {[np.asarray(o)[fin][d.argmax()] for o in operands]!r}"
        if moderate is not None and moderate[fin].any():
            dm = d[moderate[fin]]
            assert dm.max() <= POW_MODERATE_ULP, f"{name}: {int(dm.max())} ulp where |y log2 x| <= 32, at {[np.asarray(o)[fin][moderate[fin]][dm.argmax()] for o in operands]!r}"
    return int(d.max()) if d.size else 0
