"""The generated label cases of tests/_label_cover_cases.py, checked with the oracle alone (no GPU): a case can only
catch an ordering bug of k_label_cover if its f64 totals depend on the call order, and only through cells that are
neither clamped to 1.0 nor negative.  Per case:

  * every oracle total lies strictly inside (0, 1);
  * reversing the call order changes the bits of at least 5 cells (the one-call label has one order and is exempt);
  * the window (rows, columns) is the one the case was built to reach.

The status pair of tests/test_gpu_label_cover.py is proved here too: the cell is exactly 0 in call order and 2^-61 in
the reversed order."""
import numpy as np
import pytest

from tests import _label_cover_cases as lc

CASES = lc.cases()
MIN_CHANGED = 5


def _totals(oracle, segs):
    xy, t = oracle.rasterizer_pixels(segs)
    return {(int(x), int(y)): np.float64(v).view(np.uint64) for (x, y), v in zip(xy, t)}, t


def changed_cells(oracle, a, b):
    ta, _ = _totals(oracle, a)
    tb, _ = _totals(oracle, b)
    return sum(1 for k in set(ta) | set(tb) if ta.get(k) != tb.get(k))


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_is_inside_the_unit_interval_and_order_sensitive(oracle, case):
    _, t = _totals(oracle, case.segs)
    assert len(t) > 0 and (t > 0.0).all() and (t < 1.0).all(), f"{case.name}: totals outside (0, 1): max {t.max()!r}"
    if case.order_sensitive:
        n = changed_cells(oracle, case.segs, case.segs[::-1])
        assert n >= MIN_CHANGED, f"{case.name}: reversing the call order changes {n} cells"
    else:
        assert len(case.segs) == 1


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_reaches_the_window_it_was_built_for(case):
    ry0, ry1, cx0, cols = lc.window(case.segs, lc.TILE * case.scale)
    if case.rows is not None:
        assert ry1 - ry0 + 1 == case.rows
    if case.cols is not None:
        assert cols == case.cols


def test_the_cases_cover_the_shapes_the_kernel_branches_on():
    by = {c.name: c for c in CASES}
    assert [len(by[f"calls={n}"].segs) for n in (1, 63, 64, 65, 128, 129, 200)] == [1, 63, 64, 65, 128, 129, 200]
    wins = {c.name: lc.window(c.segs, lc.TILE * c.scale) for c in CASES}
    dims = {(w[1] - w[0] + 1, w[3]) for w in wins.values()}
    for rows in (1, 63, 64, 65, 130):
        assert any(r == rows and c <= 9 for r, c in dims)
    for rows in (1, 64, 65, 130):
        assert (rows, lc.LDS_CELLS + 1) in dims
    assert {c for _, c in dims} >= {288, 289, lc.LDS_CELLS}
    assert any((r * c) % 64 for r, c in dims if c <= lc.LDS_CELLS)  # a partial last word of the bit stream
    # skipped batches: the 64-call blocks alternate between two clusters more than one band apart
    segs = by["skipped-batches"].segs
    blocks = [segs[i : i + 64] for i in range(0, len(segs), 64)]
    top = [bool((b[:, 1] < 100).all()) for b in blocks]
    assert top == [True, False, True, False, True] and all((b[:, 1] < 100).all() or (b[:, 1] > 190).all() for b in blocks)
    # one cell takes every call of the first batch
    first = by["one-channel"].segs[:64]
    assert (np.floor(first[:, [0, 2]]) == 150).all() and (np.floor(first[:, [1, 3]]) == 80).all()
    # clipped windows at both scales, cut at the top and at the bottom
    for s in (1, 2):
        W = lc.TILE * s
        assert by[f"clip-top@{s}"].segs[:, [1, 3]].min() < -W and wins[f"clip-top@{s}"][0] == -W
        assert by[f"clip-bottom@{s}"].segs[:, [1, 3]].max() >= 2 * W and wins[f"clip-bottom@{s}"][1] == 2 * W - 1
        assert wins[f"clip-both@{s}"][:2] == (-W, 2 * W - 1)


def test_windowless_labels_have_no_window():
    for has_text, segs in lc.windowless_labels():
        assert lc.window(segs, lc.TILE) is None


def test_the_status_pair_turns_on_the_call_order(oracle):
    a, b = lc.status_label_a(), lc.status_label_b()
    cell = lc.STATUS_CELL
    fwd, _ = _totals(oracle, a)
    rev, _ = _totals(oracle, a[::-1])
    assert cell not in fwd and (cell[0] + 1, cell[1]) not in fwd  # exactly 0 in call order: (2^-61 + 0.25) - 0.25
    assert rev[cell] == np.float64(2.0 ** -61).view(np.uint64) and rev[(cell[0] + 1, cell[1])] == np.float64(2.0 ** -60).view(np.uint64)
    assert {k for k in fwd if k[1] == 3} == {k for k in rev if k[1] == 3} != set()  # A's own pixels, in both orders
    tb, _ = _totals(oracle, b)
    assert cell in tb and set(tb) <= {cell, (cell[0] + 1, cell[1])}
