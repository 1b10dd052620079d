"""A bounded model of Point::from_node (tile.rs:88-106, point.rs:11-19) for the projection tests.  No GPU.

The chain is restated in Python floats, one IEEE rounding per statement, in the order oracle/osm_oracle.cpp:113-145 and
csrc/osmt_project.h write it.  Its only two library calls, tan and log, are computed with mpmath at PREC bits and rounded
to the nearest double; everything else is +, -, *, / of doubles, which round the same on every IEEE machine.

x_of() therefore has no slack: the longitude path calls no library function, and its result is ONE integer.

y_interval() is what an implementation may answer whose tan is within KT ulp and whose log is within KL ulp of the
correctly rounded value.  KT and KL are NOT read off the code under test.  The device math library (ROCm device-libs,
OCML) states that its f64 functions meet the accuracy the OpenCL specification asks of a full-profile device; that table
(OpenCL C specification, "Relative error as ULPs", double precision) gives

    tan <= 5 ulp        log <= 3 ulp

glibc documents smaller errors for both (libm manual, "Known Maximum Errors in Math Functions"), so the oracle's answer
must lie in the same interval; tests/test_projection_model_cpu.py asserts that it does.

Because every step behind tan is monotonic (log increasing, PI - l decreasing, the rest increasing, round and the cast
non-decreasing), the extreme answers are among the four corner combinations (tan moved by -KT or +KT, log moved by -KL or
+KL); each is pushed through the rest of the chain, through f64::round (half away from zero) and through `as i32`
(saturating, NaN -> 0).  Exact cases get no slack: tan(+-0) = +-0, log(1) = 0, log(0) = -inf, and a NaN or an infinity
stays what it is."""
import math
import struct

import mpmath

PREC = 256  # bits; the issue asks for >= 200
KT, KL = 5, 3  # OpenCL full profile, double precision: tan <= 5 ulp, log <= 3 ulp
PI = math.pi  # 3.14159265358979323846264338327950288 rounded to a double: the constant of all three sources
TILE_SIZE = 256
I32_MAX, I32_MIN = 2147483647, -2147483648


def f2h(v):
    """a double as 16 hex digits of its bit pattern"""
    return struct.pack(">d", v).hex()


def h2f(s):
    return struct.unpack(">d", bytes.fromhex(s))[0]


def _nearest_double(v):
    """an mpf of PREC bits -> the nearest double (results here are never subnormal: |tan| >= 1e-17, |log| >= 1e-16 or 0)"""
    with mpmath.workprec(53):
        r = +v  # one rounding to 53 bits, to nearest
    f = float(r)
    assert f == 0.0 or 2.3e-308 < abs(f) < 1.7e308, f
    return f


def tan_cr(a):
    """correctly rounded tan of a double"""
    if a != a or math.isinf(a):
        return math.nan
    if a == 0.0:
        return a  # tan(+-0) = +-0
    with mpmath.workprec(PREC):
        return _nearest_double(mpmath.tan(mpmath.mpf(a)))


def log_cr(t):
    """correctly rounded log of a double"""
    if t != t or t < 0.0:
        return math.nan
    if t == 0.0:
        return -math.inf
    if math.isinf(t):
        return math.inf
    if t == 1.0:
        return 0.0
    with mpmath.workprec(PREC):
        return _nearest_double(mpmath.log(mpmath.mpf(t)))


def move_ulps(v, k):
    """v moved k doubles up (k > 0) or down (k < 0); NaN, infinities and exact zeros stay"""
    if v != v or math.isinf(v) or v == 0.0:
        return v
    to = math.inf if k > 0 else -math.inf
    for _ in range(abs(k)):
        v = math.nextafter(v, to)
    return v


def rust_round(v):
    """f64::round: half away from zero"""
    if v != v or math.isinf(v) or abs(v) >= 4503599627370496.0:
        return v
    t = float(math.trunc(v))
    if abs(v - t) >= 0.5:  # v - t is exact
        t += math.copysign(1.0, v)
    return t


def as_i32(v):
    """Rust `f64 as i32`: saturating, NaN -> 0"""
    if v != v:
        return 0
    if v >= 2147483647.0:
        return I32_MAX
    if v <= -2147483648.0:
        return I32_MIN
    return int(v)


def _dim(zoom):
    return float((TILE_SIZE * (1 << zoom)) & 0xFFFFFFFF)


def _offset(t):
    return float((t * TILE_SIZE) & 0xFFFFFFFF)


def rx_of(lon, zoom, tx):
    """the unrounded tile-relative x before the scale (pure IEEE)"""
    lon_rad = lon * (PI / 180.0)
    x = lon_rad + PI
    px = (x / (2.0 * PI)) * _dim(zoom)
    return px - _offset(tx)


def x_of(lon, zoom, tx, scale):
    return as_i32(rust_round(rx_of(lon, zoom, tx) * float(scale)))


def tan_arg(lat):
    lat_rad = lat * (PI / 180.0)
    return (PI / 4.0) + (lat_rad / 2.0)


def ry_from_log(l, zoom, ty):
    """the chain behind the log, unrounded and before the scale"""
    y = PI - l
    py = (y / (2.0 * PI)) * _dim(zoom)
    return py - _offset(ty)


def y_from_log(l, zoom, ty, scale):
    return as_i32(rust_round(ry_from_log(l, zoom, ty) * float(scale)))


def y_corners(lat, zoom, ty, scale, kt=KT, kl=KL):
    """the unrounded ry * scale of the four corner combinations"""
    t = tan_cr(tan_arg(lat))
    out = []
    for dt in (-kt, kt):
        l = log_cr(move_ulps(t, dt))
        for dl in (-kl, kl):
            out.append(ry_from_log(move_ulps(l, dl), zoom, ty) * float(scale))
    return out


def y_interval(lat, zoom, ty, scale, kt=KT, kl=KL):
    """(lo, hi): every i32 an implementation within (kt, kl) ulp may answer lies in it"""
    ys = [as_i32(rust_round(v)) for v in y_corners(lat, zoom, ty, scale, kt, kl)]
    return min(ys), max(ys)


def y_width_px(lat, zoom, ty, scale, kt=KT, kl=KL):
    """the width of the interval before rounding, in pixels of the scaled tile (nan where a corner is not finite)"""
    vs = y_corners(lat, zoom, ty, scale, kt, kl)
    if any(v != v or math.isinf(v) for v in vs):
        return math.nan
    return max(vs) - min(vs)


def y_nearest(lat, zoom, ty, scale):
    """the model's own answer with correctly rounded tan and log (kt = kl = 0)"""
    return y_interval(lat, zoom, ty, scale, 0, 0)[0]
