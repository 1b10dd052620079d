"""Generates tests/golden/projection_cases.json: projection cases over the whole admitted domain with, per case, the one
integer x and the interval [y_lo, y_hi] of tests/_projection_model.py (mpmath; no GPU).  The GPU test reads the fixture and
needs neither mpmath nor the CPU seconds; tests/test_projection_model_cpu.py regenerates it and compares byte for byte.

    python tests/golden/make_projection_cases.py          # rewrites the fixture

Everything is seeded with Python's own generator (its sequence is fixed across versions); doubles are stored as the 16
hex digits of their bit pattern.  Families:

  A  random whole domain: lat in [-85.06, 85.06], lon in [-180, 180], every zoom 0..18, a uniform tile, scales 1..4
  B  edges: the admitted limits, the square's limit, +-0, subnormals and tiny values, at the corner tiles of zooms 0, 1, 17, 18
  C  x ties: longitudes whose rx * scale has a fraction of exactly 0.5, right and left of the tile
  D  y near ties: latitudes inverted from ry * scale = k + 1/2, moved by -2..2 ulp
  E  outside the square (osmt_project only, which does not check coordinates): poles, NaN, infinities, 1e300
"""
import json
import math
import os
import random
import sys

import mpmath

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _projection_model as M  # noqa: E402

OUT = os.path.join(HERE, "projection_cases.json")
COLUMNS = ["family", "lat", "lon", "zoom", "tx", "ty", "scale", "x", "y_lo", "y_hi"]
MAX_LAT = 85.06  # OSMT_MAX_ABS_LAT
SQUARE_LAT = 85.0511287798066  # where the Mercator square ends
SEED = 20260


def case(family, lat, lon, zoom, tx, ty, scale):
    y_lo, y_hi = M.y_interval(lat, zoom, ty, scale)
    return [family, M.f2h(lat), M.f2h(lon), zoom, tx, ty, scale, M.x_of(lon, zoom, tx, scale), y_lo, y_hi]


def single(c):
    return c[8] == c[9]


def family_a(rng):
    zooms = list(range(19)) * 79  # 1501 cases, every zoom 79 times
    out = []
    for i, zoom in enumerate(zooms[:1500]):
        n = 1 << zoom
        while True:
            c = case("A", rng.uniform(-MAX_LAT, MAX_LAT), rng.uniform(-180.0, 180.0), zoom, rng.randrange(n), rng.randrange(n), 1 + i % 4)
            if single(c):  # a random point on a tie: draw again (the conditions below count on it)
                break
        out.append(c)
    return out


def corner_tiles(zoom):
    m = (1 << zoom) - 1
    return sorted({(0, 0), (m, 0), (0, m), (m, m)})


def family_b(rng):
    inf = math.inf
    lats = []
    for v in (MAX_LAT, SQUARE_LAT):
        lats += [v, -v, math.nextafter(v, 0.0), math.nextafter(-v, 0.0)]
    lats += [0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300]
    lons = [180.0, -180.0, math.nextafter(180.0, 0.0), math.nextafter(-180.0, 0.0), 0.0, -0.0, 5e-324, -5e-324]
    assert all(abs(v) <= MAX_LAT for v in lats) and all(abs(v) <= 180.0 for v in lons) and inf > 0
    full = [(la, lo, z, t, s) for la in lats for lo in lons for z in (0, 1, 17, 18) for t in corner_tiles(z) for s in (1, 4)]
    # kept whatever the thinning does: the vertices of the rendering cases (the limits, the square's corners, the equator and
    # the prime meridian under every corner tile of zooms 0 and 18 at scales 1 and 4)
    keep_lat = {M.f2h(v) for v in (MAX_LAT, -MAX_LAT, SQUARE_LAT, -SQUARE_LAT, 0.0)}
    keep_lon = {M.f2h(v) for v in (180.0, -180.0, 0.0)}
    is_kept = [M.f2h(f[0]) in keep_lat and M.f2h(f[1]) in keep_lon and f[2] in (0, 18) for f in full]
    kept = [f for f, k in zip(full, is_kept) if k]
    rest = [f for f, k in zip(full, is_kept) if not k]  # (by position: -0.0 == 0.0 as values)
    rng.shuffle(rest)
    picked = kept + rest[: 700 - len(kept)]
    # thinning must not lose a value of any factor
    for k, vals in ((0, lats), (1, lons)):
        assert {M.f2h(p[k]) for p in picked} == {M.f2h(v) for v in vals}
    assert {(p[2], p[3], p[4]) for p in picked} == {(f[2], f[3], f[4]) for f in full}
    picked.sort(key=lambda p: (p[2], p[3], p[4]))  # grouped by (zoom, tile, scale); the shuffle's order inside a group
    return [case("B", la, lo, z, t[0], t[1], s) for la, lo, z, t, s in picked]


def family_c(rng):
    out = []
    zooms = [0, 1, 5, 10, 15, 17, 18]
    for zoom in zooms:
        n = 1 << zoom
        dim = 256 * n
        for scale in (1, 2, 3, 4):
            kept = 0
            for _ in range(64):
                if kept == 8:
                    break
                tx = rng.choice([0, n - 1, rng.randrange(n)])
                left = rng.random() < 0.4
                # a world column k (in scaled pixels) right of the tile's left edge, or left of it
                k = tx * 256 * scale + (rng.randrange(-300 * scale, 0) if left else rng.randrange(0, 300 * scale))
                if not 0 <= k < dim * scale:
                    continue
                lon = -180.0 + 360.0 * (k + 0.5) / (dim * scale)
                v = M.rx_of(lon, zoom, tx) * float(scale)
                if abs(v - math.trunc(v)) != 0.5:
                    continue
                ty = rng.randrange(n)
                while True:
                    c = case("C", rng.uniform(-MAX_LAT, MAX_LAT), lon, zoom, tx, ty, scale)
                    if single(c):
                        break
                out.append(c)
                kept += 1
    return out


def lat_of_world_y(wy, dim):
    """the latitude (mpf, degrees) whose world pixel row is wy at a world of dim pixels: the formula inverted"""
    y = mpmath.mpf(wy) / dim * 2 * mpmath.pi
    t = mpmath.exp(mpmath.pi - y)
    return 2 * (mpmath.atan(t) - mpmath.pi / 4) * 180 / mpmath.pi


def family_d(rng):
    out = []
    i = 0
    while len(out) < 800:
        zoom, scale = i % 19, 1 + (i // 19) % 4
        i += 1
        n = 1 << zoom
        tx, ty = rng.randrange(n), rng.randrange(n)
        k = rng.randrange(-256 * scale, 512 * scale)
        with mpmath.workprec(M.PREC):
            wy = mpmath.mpf(ty * 256) + (mpmath.mpf(k) + mpmath.mpf(0.5)) / scale
            lat = float(lat_of_world_y(wy, 256 * n))
        lat = M.move_ulps(lat, rng.randrange(-2, 3))
        if not abs(lat) <= MAX_LAT:
            continue
        out.append(case("D", lat, rng.uniform(-180.0, 180.0), zoom, tx, ty, scale))
    return out


def family_e(rng):
    inf, nan = math.inf, math.nan
    out = []
    tiles = [(0, 0, 0), (18, 0, 0), (18, (1 << 18) - 1, (1 << 18) - 1), (15, 19807, 10243)]
    for la in (90.0, -90.0, 89.9999, -89.9999, nan, inf, -inf):
        for j in range(3):
            zoom, tx, ty = tiles[(j + len(out)) % 4]
            out.append(case("E", la, rng.uniform(-180.0, 180.0), zoom, tx, ty, (1, 4, 2)[j]))
    for lo in (nan, inf, -inf, 1e300, -1e300):
        for j in range(4):
            zoom, tx, ty = tiles[j]
            out.append(case("E", rng.uniform(-85.0, 85.0), lo, zoom, tx, ty, (1, 4, 3, 2)[j]))
    return out


def check_conditions(cases):
    """the conditions on the fixture (the CPU test asserts them again on the committed file)"""
    fam = {f: [c for c in cases if c[0] == f] for f in "ABCDE"}
    for f in "ABC":
        assert all(single(c) for c in fam[f]), f"family {f}: an interval holds two integers: change the seed"
    undecided = sum(not single(c) for c in fam["D"])
    assert 2 * undecided >= len(fam["D"]), f"family D: only {undecided} of {len(fam['D'])} undecided: not a tie set"
    assert all(0 <= c[9] - c[8] <= 1 for c in cases if c[0] != "E")
    for z in range(19):
        assert sum(c[3] == z for c in fam["A"]) >= 50
    assert {c[6] for c in fam["A"]} == {1, 2, 3, 4} and 1400 <= len(fam["A"]) <= 1600
    assert 0 < len(fam["B"]) <= 800
    assert len(fam["C"]) >= 100 and len({c[3] for c in fam["C"]}) >= 6
    assert sum(M.rx_of(M.h2f(c[2]), c[3], c[4]) < 0 for c in fam["C"]) >= 20
    for c in fam["C"]:
        v = M.rx_of(M.h2f(c[2]), c[3], c[4]) * float(c[6])
        assert abs(v - math.trunc(v)) == 0.5
    assert 700 <= len(fam["D"]) <= 900 and {c[3] for c in fam["D"]} == set(range(19)) and {c[6] for c in fam["D"]} == {1, 2, 3, 4}
    assert 30 <= len(fam["E"]) <= 50
    return {f: len(v) for f, v in fam.items()}, undecided


def generate():
    """the fixture's text"""
    rng = random.Random(SEED)
    cases = family_a(rng) + family_b(rng) + family_c(rng) + family_d(rng) + family_e(rng)
    check_conditions(cases)
    head = {"model": "tests/_projection_model.py", "kt_ulp": M.KT, "kl_ulp": M.KL, "seed": SEED, "columns": COLUMNS}
    lines = ",\n".join(json.dumps(c, separators=(",", ":")) for c in cases)
    return json.dumps(head, separators=(",", ":"))[:-1] + ',"cases":[\n' + lines + "\n]}\n"


if __name__ == "__main__":
    text = generate()
    assert len(text) < 300 * 1000, len(text)
    with open(OUT, "w") as f:
        f.write(text)
    counts, undecided = check_conditions(json.loads(text)["cases"])
    print(f"{OUT}: {len(text)} bytes, cases {counts}, {undecided} of family D undecided")
