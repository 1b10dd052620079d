"""The projection fixture (tests/golden/projection_cases.json) against its generator, the oracle and the factor-built
projection of the label anchors.  The model (tests/_projection_model.py) gives one integer x — the longitude path calls no
library function — and an interval for y derived from stated ULP bounds of tan and log; glibc's documented errors are
smaller than those bounds, so the oracle must answer x exactly and y inside the interval.  No GPU."""
import importlib.util
import math
import os

import numpy as np

from tests import _anchors as A
from tests import _projection_cases as PC
from tests import _projection_model as M


def _generator():
    path = os.path.join(os.path.dirname(PC.PATH), "make_projection_cases.py")
    spec = importlib.util.spec_from_file_location("make_projection_cases", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_regenerates_byte_for_byte():
    with open(PC.PATH, "rb") as f:
        have = f.read()
    assert len(have) < 300 * 1000
    assert _generator().generate().encode() == have


def test_fixture_conditions():
    cs = PC.load()
    fam = {f: cs[cs["family"] == f] for f in "ABCDE"}
    assert sum(len(v) for v in fam.values()) == len(cs)
    for f in "ABC":  # one fixed integer: these families are asserted equal to the oracle
        assert (fam[f]["y_lo"] == fam[f]["y_hi"]).all()
    d = fam["D"]
    assert 2 * int((d["y_lo"] < d["y_hi"]).sum()) >= len(d)  # a tie set
    inside = cs[cs["family"] != "E"]
    w = inside["y_hi"].astype(np.int64) - inside["y_lo"]
    assert (w >= 0).all() and (w <= 1).all()
    # what the issue asks of the families
    assert all(int((fam["A"]["zoom"] == z).sum()) >= 50 for z in range(19)) and set(fam["A"]["scale"]) == {1, 2, 3, 4}
    assert (np.abs(inside["lat"]) <= 85.06).all() and (np.abs(inside["lon"]) <= 180.0).all()
    assert len(fam["C"]) >= 100 and len(set(fam["C"]["zoom"])) >= 6
    rx = np.array([M.rx_of(c["lon"], int(c["zoom"]), int(c["tx"])) for c in fam["C"]])
    v = rx * fam["C"]["scale"]
    assert (np.abs(v - np.trunc(v)) == 0.5).all() and int((rx < 0).sum()) >= 20
    b = fam["B"]
    assert {85.06, -85.06, 0.0, 5e-324, -5e-324, 1e-300, -1e-300} <= set(b["lat"]) and {180.0, -180.0, 5e-324, -5e-324} <= set(b["lon"])
    assert any(math.copysign(1.0, v) < 0 and v == 0.0 for v in b["lat"]) and any(math.copysign(1.0, v) < 0 and v == 0.0 for v in b["lon"])
    assert int((b["x"] < 0).sum()) > 0 and int((b["y_lo"] < 0).sum()) > 0  # a corner tile opposite the point
    assert set(d["zoom"]) == set(range(19)) and set(d["scale"]) == {1, 2, 3, 4}
    e = fam["E"]
    assert np.isnan(e["lat"]).any() and np.isinf(e["lat"]).any() and np.isnan(e["lon"]).any() and np.isinf(e["lon"]).any()
    assert (e["y_lo"][np.isnan(e["lat"]) | np.isinf(e["lat"])] == 0).all() and (e["x"][np.isnan(e["lon"])] == 0).all()
    assert {M.I32_MAX, M.I32_MIN} <= set(e["x"]) and M.I32_MAX in set(e["y_lo"])  # saturation on both axes


def test_model_agrees_with_the_fixture_columns():
    """the stored x and interval are the model's (a spot check beside the byte comparison, through the reader)"""
    cs = PC.load()
    for c in cs[:: max(1, len(cs) // 200)]:
        z, tx, ty, s = int(c["zoom"]), int(c["tx"]), int(c["ty"]), int(c["scale"])
        assert M.x_of(float(c["lon"]), z, tx, s) == c["x"]
        assert M.y_interval(float(c["lat"]), z, ty, s) == (c["y_lo"], c["y_hi"])


def test_interval_width_before_rounding():
    """the figure DESIGN 3.1 and include/osmtile.h quote: with tan within 5 ulp and log within 3 ulp the unrounded ry * scale
    moves by at most 2.4e-7 px over the admitted domain — four ulp of a coordinate near 2^28, reached at zoom 18 and scale 4"""
    cs = PC.load()
    inside = cs[cs["family"] != "E"]
    w = np.array([M.y_width_px(float(c["lat"]), int(c["zoom"]), int(c["ty"]), int(c["scale"])) for c in inside])
    top = inside[int(np.argmax(w))]
    print(f"\nwidest interval before rounding: {w.max()!r} px at zoom {top['zoom']}, scale {top['scale']}, lat {top['lat']!r}")
    assert np.isfinite(w).all() and 0.0 < w.max() <= 4 * 2.0 ** -24  # 4 ulp of [2^28, 2^29): 2.384e-7
    assert top["zoom"] == 18 and top["scale"] == 4
    assert w[inside["zoom"] <= 10].max() < 1e-9


def test_oracle_x_is_the_model_and_y_lies_in_the_interval(oracle):
    cs = PC.load()
    ll = PC.latlon(cs)
    for (z, tx, ty, s), idx in PC.groups(cs).items():
        got = oracle.project_points(ll[idx], z, tx, ty, float(s))
        c = cs[idx]
        assert np.array_equal(got[:, 0], c["x"]), (z, tx, ty, s)
        assert ((c["y_lo"] <= got[:, 1]) & (got[:, 1] <= c["y_hi"])).all(), (z, tx, ty, s)


def test_project_from_factors_x_is_the_model_and_y_lies_in_the_interval():
    """osmt::mercator_factors and the three exact operations of the anchors, then f64::round and `as i32`"""
    cs = PC.load()
    f = A.mercator_factors(PC.latlon(cs))
    for i, c in enumerate(cs):
        p = A.np_project(f[i], int(c["zoom"]), int(c["tx"]), int(c["ty"]), int(c["scale"]))[0]
        x, y = M.as_i32(M.rust_round(float(p[0]))), M.as_i32(M.rust_round(float(p[1])))
        assert x == c["x"], (i, c)
        assert c["y_lo"] <= y <= c["y_hi"], (i, c)
