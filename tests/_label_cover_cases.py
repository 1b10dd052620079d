"""Label cases for the coverage-plane tests (tests/test_label_cover_cases_cpu.py, tests/test_gpu_label_cover.py).

k_label_cover exists to give every cell its f64 addends in draw_line call order (the reference's per-key sums do not
associate), so a case is only worth rendering if its totals DEPEND on that order.  Random open segments do not: their
totals go negative or clamp to 1.0.  The cases here are built from

  * closed triangles (and a quad / pentagon where a call count needs one) of positive coverage: the left boundary is
    walked towards +y (font/rasterizer.rs:34), i.e. the shoelace sum in y-down coordinates is negative;
  * circumradius about 0.35 px, at most three centres per cell, so that several overlap in a cell and the totals stay
    inside (0, 1) — never clamped;
  * unaligned f64 coordinates;
  * a share of slivers 2.5 .. 6 px long and 0.06 px wide: three stripes tall or three cells wide, the calls the kernel
    replays stripe by stripe instead of parking them in a channel.

Each case is ONE label (its draw_line calls, float64 [n, 4]) with the window it must get.  The shapes come from the
kernel (osmt_labels.hip): batches of 64 calls, bands of min(64, 576 / cols) stripes, k_label_cover_wide from 577
columns on.  The CPU test proves with the oracle alone that every case has its totals strictly inside (0, 1) and that
reversing its call order changes the bits of at least five cells; the GPU test then asks for the oracle's bits.

The window of a label (osmt_label_extent_add, osmt_glyph.h): rows = the stripes of its non-horizontal calls clipped to
[-W, 2W), columns = floor(min x) - 2 .. floor(max x) + 3 of the calls that have a stripe left."""
import functools
import math

import numpy as np

TILE = 256
LDS_CELLS = 576  # OSMT_LABEL_LDS_CELLS


class Case:
    def __init__(self, name, segs, scale=1, rows=None, cols=None, order_sensitive=True):
        self.name, self.scale = name, scale
        self.segs = np.ascontiguousarray(segs, dtype=np.float64).reshape(-1, 4)
        self.rows, self.cols = rows, cols  # what the case was built to get (None: whatever comes out)
        self.order_sensitive = order_sensitive

    def __repr__(self):
        return f"Case({self.name}, {len(self.segs)} calls)"


def window(segs, W):
    """osmt_label_extent_add over a label's calls: (ry0, ry1, cx0, cols), or None for a label without a window."""
    ry0 = cx0 = 1 << 30
    ry1 = cx1 = -(1 << 30)
    for x0, y0, x1, y1 in np.asarray(segs, dtype=np.float64).reshape(-1, 4):
        if y1 - y0 == 0.0:
            continue
        a, b = max(math.floor(min(y0, y1)), -W), min(math.floor(max(y0, y1)), 2 * W - 1)
        if a > b:
            continue
        ry0, ry1 = min(ry0, a), max(ry1, b)
        cx0, cx1 = min(cx0, math.floor(min(x0, x1)) - 2), max(cx1, math.floor(max(x0, x1)) + 3)
    return None if ry0 > ry1 else (ry0, ry1, cx0, cx1 - cx0 + 1)


# ---- shapes ---------------------------------------------------------------------------------------------------------
def closed(pts):
    """The draw_line calls of a closed contour, oriented for positive coverage."""
    pts = [(float(x), float(y)) for x, y in pts]
    nxt = pts[1:] + pts[:1]
    if sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(pts, nxt)) > 0.0:
        pts = pts[::-1]
        nxt = pts[1:] + pts[:1]
    return [(x0, y0, x1, y1) for (x0, y0), (x1, y1) in zip(pts, nxt)]


def ngon(rng, cx, cy, r, n=3):
    t0 = float(rng.uniform(0.0, 2.0 * math.pi))
    return closed([(cx + r * math.cos(t0 + 2.0 * math.pi * k / n), cy + r * math.sin(t0 + 2.0 * math.pi * k / n)) for k in range(n)])


def sliver(cx, cy, length, angle, width=0.06):
    """A closed rectangle length x width around (cx, cy), its long side at `angle` (0 = along x)."""
    ux, uy = math.cos(angle) * length / 2.0, math.sin(angle) * length / 2.0
    vx, vy = -math.sin(angle) * width / 2.0, math.cos(angle) * width / 2.0
    return closed([(cx - ux - vx, cy - uy - vy), (cx + ux - vx, cy + uy - vy), (cx + ux + vx, cy + uy + vy), (cx - ux + vx, cy - uy + vy)])


def reverse_calls(calls):
    """The same contour walked the other way: negative coverage."""
    return [(x1, y1, x0, y0) for x0, y0, x1, y1 in calls][::-1]


def pin(x, y):
    """A tiny triangle inside cell (x, y): fixes an end of the window without covering anything to speak of."""
    return closed([(x + 0.31, y + 0.27), (x + 0.43, y + 0.33), (x + 0.36, y + 0.46)])


def scatter(rng, x0, y0, nx, ny, n_shapes, sliver_frac=0.1, cap=3, r=0.35):
    """n_shapes shapes with their centres in the cells [x0, x0 + nx) x [y0, y0 + ny), at most `cap` centres per cell;
    every vertex stays inside the cells' area (so the window is the caller's to fix).  Returns a list of shapes (each a
    list of calls)."""
    cnt, out = {}, []
    assert n_shapes <= cap * nx * ny
    while len(out) < n_shapes:
        cx, cy = float(rng.uniform(x0, x0 + nx)), float(rng.uniform(y0, y0 + ny))
        key = (math.floor(cx), math.floor(cy))
        if cnt.get(key, 0) >= cap:
            continue
        if rng.random() < sliver_frac and (nx >= 4 or ny >= 4):
            length = float(rng.uniform(2.5, min(6.0, max(nx, ny) - 0.2)))
            tall = ny >= 4 and (nx < 4 or rng.random() < 0.5)
            ang = (math.pi / 2.0 if tall else 0.0) + float(rng.uniform(-0.12, 0.12))
            s = sliver(cx, cy, length, ang)
        else:
            s = ngon(rng, cx, cy, float(rng.uniform(0.85, 1.1)) * r)
        if all(x0 <= v[0] < x0 + nx and y0 <= v[1] < y0 + ny for v in s):
            cnt[key] = cnt.get(key, 0) + 1
            out.append(s)
    return out


def flat(shapes):
    return [c for s in shapes for c in s]


def shuffled(rng, calls):
    """Call-level shuffle: the contours stay closed (the sums do not care which call came from which shape), and the
    calls that meet in a cell come from different shapes in no particular order."""
    calls = list(calls)
    return [calls[i] for i in rng.permutation(len(calls))]


def shapes_for_calls(rng, x0, y0, nx, ny, n_calls):
    """Closed shapes with exactly n_calls calls: triangles, plus one quad or pentagon for the remainder."""
    extra = {0: [], 1: [4], 2: [5]}[n_calls % 3]
    n_tri = (n_calls - sum(extra)) // 3
    shapes = scatter(rng, x0, y0, nx, ny, n_tri, sliver_frac=0.0)
    for n in extra:
        shapes.append(ngon(rng, x0 + nx / 2.0 + 0.13, y0 + ny / 2.0 + 0.21, 0.33, n))
    assert sum(len(s) for s in shapes) == n_calls
    return shapes


# ---- the cases ------------------------------------------------------------------------------------------------------
def _call_counts():
    out = [Case("calls=1", [(40.37, 33.21, 40.81, 33.74)], rows=1, cols=6, order_sensitive=False)]  # one call has one order
    for n, side, seed in [(63, 3, 2), (64, 3, 1), (65, 3, 1), (128, 4, 4), (129, 4, 5), (200, 5, 6)]:
        rng = np.random.default_rng(1000 + seed)
        calls = shuffled(rng, flat(shapes_for_calls(rng, 30, 50, side, side, n)))
        out.append(Case(f"calls={n}", calls))
    return out


def _skipped_batches():
    """Two clusters 190 rows apart, in blocks of 64 calls A B A B A: the band of A is handed batches 0, 2, 4 and never
    1 or 3 (`if (!rest) continue` does not advance the hand-over count), the band of B batches 1 and 3."""
    rng = np.random.default_rng(2001)
    a = shuffled(rng, flat(shapes_for_calls(rng, 70, 10, 5, 5, 192)))
    b = shuffled(rng, flat(shapes_for_calls(rng, 71, 200, 4, 5, 128)))
    calls = a[:64] + b[:64] + a[64:128] + b[64:] + a[128:]
    return [Case("skipped-batches", calls)]


def _framed(rng, x, y, cols, rows, clusters, sliver_frac=0.1):
    """Calls of a window of exactly rows x cols cells whose first cell column holding a vertex is x and first stripe
    is y: pins at the corners, `clusters` = [(dx, dy, nx, ny, n_shapes)] in cells relative to (x, y)."""
    span = cols - 6  # floor(max x) - floor(min x)
    assert span >= 0
    shapes = [pin(x, y), pin(x + span, y + rows - 1)]
    for dx, dy, nx, ny, n in clusters:
        assert 0 <= dx and dx + nx <= span + 1 and 0 <= dy and dy + ny <= rows
        if ny == 1:  # one stripe: smaller shapes, more of them per cell
            shapes += scatter(rng, x + dx, y + dy, nx, ny, n, sliver_frac=sliver_frac, cap=6, r=0.24)
        else:
            shapes += scatter(rng, x + dx, y + dy, nx, ny, n, sliver_frac=sliver_frac)
    return shapes


def _band_geometry():
    out = []
    # cols <= 9: bands of 64 stripes; 1, 63, 64, 65, 130 rows (one band, one short of full, full, one stripe into the
    # second, two full bands and two stripes); 7 or 9 columns so that rows x cols is mostly no multiple of 64
    for rows, cols, seed in [(1, 9, 1), (63, 7, 2), (64, 9, 3), (65, 7, 4), (130, 9, 5)]:
        rng = np.random.default_rng(3000 + seed)
        nx = cols - 5
        if rows == 1:
            cl = [(0, 0, nx, 1, 6 * nx)]
        elif rows < 70:
            cl = [(0, 0, nx, 5, 20), (0, 56, nx, rows - 56, 30)]  # the second one across the first band's last stripes
        else:
            cl = [(0, 0, nx, 5, 20), (0, 58, nx, 12, 40), (0, 120, nx, 10, 40)]  # across stripes 63 / 64 and 127 / 128
        # one stripe of nine columns has five cells a call can reach, and all five must be order-sensitive: in stripe 0
        # the y values span binades, so the S sums (differences of y, exact inside one binade) round as well
        y = 0 if rows == 1 else 40
        shapes = _framed(rng, 20, y, cols, rows, cl)
        if rows == 130:
            # calls that cross the band edge at stripe 63 / 64: two stripes on either side (parked in both bands), and
            # three stripes in the first band (replayed there) with two in the second (parked)
            shapes.append(sliver(21.3, y + 64.02, 3.6, math.pi / 2 + 0.05))
            shapes.append(sliver(22.6, y + 63.6, 4.7, math.pi / 2 - 0.04))
        out.append(Case(f"band-{rows}x{cols}", shuffled(rng, flat(shapes)), rows=rows, cols=cols))
    # 288 columns: two stripes per band; 289: one; 576: the last streamed width; each with a partial last band or
    # more than one band, and calls five stripes tall that cross three bands
    for rows, cols, seed in [(5, 288, 6), (4, 289, 7), (3, 576, 8)]:
        rng = np.random.default_rng(3000 + seed)
        span = cols - 6
        cl = [(0, 0, 6, rows, 24), (span - 5, 0, 6, rows, 24), (span // 2, 0, 8, rows, 30)]
        shapes = _framed(rng, -40, 100, cols, rows, cl, sliver_frac=0.15)
        if rows >= 4:
            shapes.append(sliver(-40 + span // 2 + 3.4, 100 + rows / 2.0, rows - 0.3, math.pi / 2 + 0.07))
        out.append(Case(f"band-{rows}x{cols}", shuffled(rng, flat(shapes)), rows=rows, cols=cols))
    # 577 columns: k_label_cover_wide; 1, 64, 65, 130 rows (its S scratch is reused for every round of 64 rows)
    for rows, seed in [(1, 9), (64, 10), (65, 11), (130, 12)]:
        rng = np.random.default_rng(3000 + seed)
        span = 577 - 6
        if rows == 1:
            cl = [(0, 0, 5, 1, 12), (span - 4, 0, 5, 1, 12)]
        else:
            cl = [(0, 0, 5, 4, 20), (span - 4, rows - 4, 5, 4, 20), (300, rows - 6, 5, 6, 24)]
            if rows == 130:
                cl.append((100, 60, 5, 8, 30))  # across the first round's last stripes
        shapes = _framed(rng, -150, 60, 577, rows, cl)
        out.append(Case(f"wide-{rows}x577", shuffled(rng, flat(shapes)), rows=rows, cols=577))
    return out


def _replay_between_channel_sums():
    """One batch in which a short call, a sliver and another short call add to the same cell, the sliver three stripes
    tall in one case and three cells wide in the other: the replay has to land between the two channel sums."""
    out = []
    for name, ang, seed in [("tall", math.pi / 2 + 0.06, 1), ("wide", 0.05, 2)]:
        rng = np.random.default_rng(4000 + seed)
        cx, cy = 90.47, 120.52  # the cell (90, 120)
        core = flat([ngon(rng, cx - 0.05, cy + 0.03, 0.3), sliver(cx, cy, 3.4, ang), ngon(rng, cx + 0.06, cy - 0.04, 0.3),
                     sliver(cx + 0.11, cy + 0.07, 4.2, ang + 0.02), ngon(rng, cx, cy, 0.25)])
        rest = shuffled(rng, flat(scatter(rng, 87, 117, 7, 7, 60, sliver_frac=0.2, cap=2)))
        out.append(Case(f"replay-{name}", core + rest))
    return out


def _one_cell():
    """All 64 calls of the first batch inside ONE cell (one chain of A sums, one of S sums), and the same load around a
    corner of four cells (all eight channels); a scattered cluster behind them."""
    out = []
    for name, (cx, cy), r, seed in [("one-channel", (150.5, 80.5), 0.13, 1), ("eight-channels", (151.0, 81.0), 0.26, 2)]:
        rng = np.random.default_rng(5000 + seed)
        shapes = []
        for k in range(21):
            n = 4 if k == 20 else 3
            j = 0.3 if name == "one-channel" else 0.12
            shapes.append(ngon(rng, cx + float(rng.uniform(-j, j)), cy + float(rng.uniform(-j, j)), r * float(rng.uniform(0.6, 1.0)), n))
        first = shuffled(rng, flat(shapes))
        assert len(first) == 64
        if name == "one-channel":
            assert all(math.floor(v) == 150 for c in first for v in (c[0], c[2])) and all(math.floor(v) == 80 for c in first for v in (c[1], c[3]))
        rest = shuffled(rng, flat(scatter(rng, 147, 78, 3, 6, 30, sliver_frac=0.0) + scatter(rng, 152, 78, 3, 6, 30, sliver_frac=0.0)))
        out.append(Case(name, first + rest))
    return out


def _cancellation():
    """Contours and, later in the order, the same contours walked the other way: the cells end at 0 or at a residue of
    either sign.  Axis-parallel rectangles cancel exactly (a vertical call's areas do not depend on its direction) and
    bring the horizontal calls (delta == 0, draw_line returns at once) in between.  A positive cluster on top keeps the
    case order-sensitive."""
    rng = np.random.default_rng(6001)
    pos = scatter(rng, 200, 30, 5, 5, 30, sliver_frac=0.15)
    neg = [reverse_calls(s) for s in pos]
    rects = []
    for _ in range(8):
        x, y = float(rng.uniform(200, 204)), float(rng.uniform(30, 34))
        w, h = float(rng.uniform(0.2, 0.9)), float(rng.uniform(0.2, 0.9))
        rects.append(closed([(x, y), (x + w, y), (x + w, y + h), (x, y + h)]))
    horiz = [(200.3, 31.7, 204.1, 31.7), (203.9, 33.25, 201.2, 33.25)]
    calls = flat(pos[:15]) + flat(rects[:4]) + horiz[:1] + flat(neg[:15]) + [c for r in rects[:4] for c in reverse_calls(r)]
    calls += shuffled(rng, flat(pos[15:]) + flat(neg[15:]) + flat(rects[4:]) + [c for r in rects[4:] for c in reverse_calls(r)] + horiz[1:])
    calls += shuffled(rng, flat(scatter(rng, 200, 30, 5, 5, 45, sliver_frac=0.1)))
    return [Case("cancellation", calls)]


def _clipping():
    """Windows cut by the label area's rows [-W, 2W): stripes above -W and from 2W on are no rows of the plane."""
    out = []
    for scale in (1, 2):
        W = TILE * scale
        rng = np.random.default_rng(7000 + scale)
        top = flat(scatter(rng, 33, -W - 4, 4, 8, 60, sliver_frac=0.2))
        bot = flat(scatter(rng, 35, 2 * W - 4, 4, 8, 60, sliver_frac=0.2))
        out.append(Case(f"clip-top@{scale}", shuffled(rng, top), scale=scale, rows=4))
        out.append(Case(f"clip-bottom@{scale}", shuffled(rng, bot), scale=scale, rows=4))
        out.append(Case(f"clip-both@{scale}", shuffled(rng, top + bot), scale=scale, rows=3 * W))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """Every generated case, in a fixed order (tuple of Case)."""
    return tuple(_call_counts() + _skipped_batches() + _band_geometry() + _replay_between_channel_sums() + _one_cell()
                 + _cancellation() + _clipping())


def windowless_labels():
    """Labels that have no window: (has_text, segs) — no text, a text without calls, calls outside the label area's
    rows, only horizontal calls."""
    far = np.array(closed([(10.2, -300.7), (11.1, -300.2), (10.4, -299.6)]))
    below = np.array(closed([(10.2, 600.7), (11.1, 600.2), (10.4, 601.6)]))
    return [(0, np.zeros((0, 4))), (1, np.zeros((0, 4))), (1, far), (1, below), (1, np.array([(3.5, 7.25, 9.5, 7.25)]))]


# ---- the status pair ------------------------------------------------------------------------------------------------
STATUS_CELL = (40, 0)


def status_label_a():
    """Label A of the status test.  Into cell (40, 0) it adds, in call order, 2^-61 (a vertical call 2^-60 tall, half a
    cell from the right edge), then 0.25, then -0.25: (2^-61 + 0.25) - 0.25 = 0 exactly, since 0.25 absorbs 2^-61; in
    the reversed order (-0.25 + 0.25) + 2^-61 = 2^-61 > 0.  The S sums of cell (41, 0) go the same way.  A triangle in
    stripe 3 gives the label pixels of its own in both orders."""
    t = 2.0 ** -60
    calls = [(40.5, 0.0, 40.5, t), (40.5, 0.25, 40.5, 0.75), (40.5, 0.75, 40.5, 0.25)]
    return np.array(calls + closed([(44.2, 3.1), (44.9, 3.4), (44.3, 3.8)]), dtype=np.float64)


def status_label_b():
    """Label B: a triangle inside cell (40, 0) — it can only collide with A there (and in (41, 0), where its own S
    residue may leave a tiny total)."""
    return np.array(closed([(40.2, 0.2), (40.8, 0.3), (40.4, 0.8)]), dtype=np.float64)


# ---- what the GPU tests ask of a plane ------------------------------------------------------------------------------
def check_plane(scene, oracle, index, segs, W, what):
    """Label `index` of the scene's attached batch, whose draw_line calls are `segs`: the window is the one
    osmt_label_extent_add gives, every oracle pixel of a row inside [-W, 2W) lies in it and the plane holds the identical
    64-bit pattern there, and no other cell is > 0.  A label without a window reports zero rows.  Returns the plane."""
    ry0, cx0, plane = scene.read_label_cover(index)
    win = window(segs, W)
    if win is None:
        assert plane.shape[0] == 0, f"{what}: a label without a window reports {plane.shape}"
        return plane
    assert (ry0, ry0 + plane.shape[0] - 1, cx0, plane.shape[1]) == win, f"{what}: window {(ry0, cx0) + plane.shape}, expected {win}"
    xy, tot = oracle.rasterizer_pixels(segs)
    keep = (xy[:, 1] >= -W) & (xy[:, 1] < 2 * W)
    r, c, tot = xy[keep, 1] - ry0, xy[keep, 0] - cx0, tot[keep]
    assert ((r >= 0) & (r < plane.shape[0]) & (c >= 0) & (c < plane.shape[1])).all(), f"{what}: an oracle pixel lies outside the window"
    want = np.zeros(plane.shape, dtype=np.float64)
    want[r, c] = tot
    hit = np.zeros(plane.shape, dtype=bool)
    hit[r, c] = True
    bad = hit & (plane.view(np.uint64) != want.view(np.uint64))
    if bad.any():
        br, bc = (int(v[0]) for v in np.nonzero(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {int(hit.sum())} cells differ from the oracle's bits; first at (x, y) = "
                             f"({cx0 + bc}, {ry0 + br}): plane {plane[br, bc]!r} ({plane[br, bc].hex()}), oracle {want[br, bc]!r} ({want[br, bc].hex()})")
    extra = ~hit & (plane > 0.0)
    assert not extra.any(), f"{what}: {int(extra.sum())} cells are > 0 where the oracle sets no pixel"
    return plane
