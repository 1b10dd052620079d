"""The device hypot of the glyph walk (osm_renderer_amd/csrc/osmt_glyph.h), built for the host, against the libm of the
machine the test runs on: f64::hypot is that libm's hypot, and draw_quad's flatness test (font/rasterizer.rs:90-100)
compares sums of three of them, so a single differing bit can change a glyph's draw_line calls.  10^7+ inputs over
the ranges glyph outlines produce and the edges of the algorithm: 0 mismatching bits."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np

from osm_renderer_amd import labels
from tests import _glyph_shim


def _pairs(rng):
    n = 1_000_000
    u = lambda: rng.random(n)  # noqa: E731
    out = []
    out.append((u() * 64.0, u() * 64.0))  # glyph-range |dx|, |dy| at text sizes
    out.append((u() * 4096.0, u() * 4096.0))  # font units / @2x
    out.append((np.floor(u() * 2048) / 4.0, np.floor(u() * 2048) / 4.0))  # quarter-pixel grid
    out.append((np.floor(u() * 4096) / 8.0, np.floor(u() * 64) / 8.0))  # eighth-pixel grid, flat
    e = lambda lo, hi: 10.0 ** (lo + (hi - lo) * u())  # noqa: E731
    out.append((e(-8, 4), e(-8, 4)))  # 1e-8 .. 1e4, log-uniform
    x = e(-3, 3)
    out.append((x, x.copy()))  # x == y
    out.append((x, x * (1.0 + u() * 1e-9)))  # nearly equal
    out.append((e(-3, 3), np.zeros(n)))  # one zero
    out.append((np.ldexp(u(), -1074 + rng.integers(0, 60, n)), np.ldexp(u(), -1074 + rng.integers(0, 60, n))))  # subnormal
    out.append((np.ldexp(u(), rng.integers(-1022, 1024, n)), np.ldexp(u(), rng.integers(-1022, 1024, n))))  # all exponents
    out.append((np.ldexp(1.0 + u(), rng.integers(500, 1024, n)), np.ldexp(1.0 + u(), rng.integers(400, 1024, n))))  # huge (> 2^511)
    bits = rng.integers(0, 0x7FF0000000000000, size=(n, 2), dtype=np.int64).view(np.float64)  # any finite positive
    out.append((bits[:, 0], bits[:, 1] * np.where(u() < 0.5, -1.0, 1.0)))
    x = e(0, 3)
    out.append((x, x * 2.0 ** -54 * (0.5 + u())))  # around the 2^-54 early-out
    return out


def test_device_hypot_equals_host_libm_on_ten_million_inputs():
    L = _glyph_shim.lib()
    rng = np.random.default_rng(20261016)
    total = bad = 0
    for a, b in _pairs(rng):
        xy = np.ascontiguousarray(np.stack([a, b], axis=1), dtype=np.float64)
        bad += L.shim_hypot_mismatches(xy.ctypes.data_as(C.POINTER(C.c_double)), len(xy))
        total += len(xy)
    assert total >= 10_000_000
    assert bad == 0, f"{bad} of {total} inputs differ from libm's hypot"


def test_specials_and_the_python_binding_agree():
    L = _glyph_shim.lib()
    inf, nan = float("inf"), float("nan")
    cases = [(0.0, 0.0), (-0.0, 0.0), (-3.0, 4.0), (inf, nan), (nan, -inf), (nan, 1.0), (5e-324, 5e-324), (1.7976931348623157e308, 1.7976931348623157e308)]
    xy = np.array(cases, dtype=np.float64)
    got = np.empty(len(xy))
    L.shim_hypot(xy.ctypes.data_as(C.POINTER(C.c_double)), len(xy), got.ctypes.data_as(C.POINTER(C.c_double)))
    want = np.array([labels._libm.hypot(a, b) for a, b in cases])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64))
    # the host twin (labels.flatten_quad) calls the same libm through ctypes
    rng = np.random.default_rng(3)
    a, b = rng.random(2000) * 50, rng.random(2000) * 50
    xy = np.ascontiguousarray(np.stack([a, b], axis=1))
    got = np.empty(2000)
    L.shim_hypot(xy.ctypes.data_as(C.POINTER(C.c_double)), 2000, got.ctypes.data_as(C.POINTER(C.c_double)))
    assert np.array_equal(got, np.array([labels._libm.hypot(x, y) for x, y in zip(a, b)]))


def _correctly_rounded_hypot(x, y):
    """The double nearest to sqrt(x^2 + y^2), decided exactly: candidate c is it iff the exact sum lies between the
    squares of the midpoints to its neighbours."""
    S = Fraction(x) ** 2 + Fraction(y) ** 2
    c = math.sqrt(float(S))
    for cand in (c, math.nextafter(c, 0.0), math.nextafter(c, math.inf)):
        lo = (Fraction(cand) + Fraction(math.nextafter(cand, 0.0))) / 2
        hi = (Fraction(cand) + Fraction(math.nextafter(cand, math.inf))) / 2
        if lo * lo <= S <= hi * hi:
            return cand
    raise AssertionError("no candidate")


def test_the_naive_formula_is_not_enough():
    """Why the restatement exists: neither sqrt(x*x + y*y) nor a correctly rounded hypot is libm's (on glyph-range
    inputs), while the restatement is (test above)."""
    rng = np.random.default_rng(5)
    a, b = rng.random(300_000) * 64, rng.random(300_000) * 64
    naive = np.sqrt(a * a + b * b)
    assert (naive != np.hypot(a, b)).sum() > 0
    n = 20_000
    cr = np.array([_correctly_rounded_hypot(float(x), float(y)) for x, y in zip(a[:n], b[:n])])
    libm = np.array([labels._libm.hypot(float(x), float(y)) for x, y in zip(a[:n], b[:n])])
    assert (cr != libm).sum() > 0, "libm's hypot is correctly rounded here: the restatement would not be needed"
    assert (np.abs(cr - libm) <= np.spacing(cr)).all()  # within one ulp
