"""A second, independent statement of the label-position function (the reference's get_label_position for ways and
multipolygons, src/draw/labelable.rs:191-204) in plain Python: floats are IEEE f64, math.sqrt is correctly rounded, every
expression keeps the reference's association.  The priority queue is std::collections::BinaryHeap restated (push: append
and sift up while NOT <= the parent; pop: last element to the root, hole to the bottom taking the right child when
left <= right, then sift up) — `tie="std"`.  `tie="other"` is a correct max-heap that breaks ties the other way
(heapq on (-key, -sequence number): of equal keys the one pushed LAST comes out first); the tests use it to show that the
tie order matters on symmetric shapes.

Also the seeded request families the CPU and GPU tests share.
"""
import heapq
import math
import struct

import numpy as np

OK, NONE, TOO_LARGE = 0, 1, 2
MAX_CELLS = 65536
SQRT_2 = 1.4142135623730951
INF = float("inf")


class _StdHeap:
    def __init__(self):
        self.d = []

    def __len__(self):
        return len(self.d)

    def _sift_up(self, start, pos):
        d = self.d
        e = d[pos]
        while pos > start:
            parent = (pos - 1) // 2
            if not (e[0] > d[parent][0]):  # e <= parent
                break
            d[pos] = d[parent]
            pos = parent
        d[pos] = e

    def push(self, cell):
        self.d.append(cell)
        self._sift_up(0, len(self.d) - 1)

    def pop(self):
        d = self.d
        item = d.pop()
        if d:
            item, d[0] = d[0], item
            end = len(d)
            e = d[0]
            pos, child = 0, 1
            while child <= max(end - 2, 0):  # end.saturating_sub(2)
                if not (d[child][0] > d[child + 1][0]):
                    child += 1
                d[pos] = d[child]
                pos = child
                child = 2 * pos + 1
            if child == end - 1:
                d[pos] = d[child]
                pos = child
            d[pos] = e
            self._sift_up(0, pos)
        return item


class _OtherHeap:
    def __init__(self):
        self.d = []
        self.seq = 0

    def __len__(self):
        return len(self.d)

    def push(self, cell):
        self.seq += 1
        heapq.heappush(self.d, (-cell[0], -self.seq, cell))

    def pop(self):
        return heapq.heappop(self.d)[2]


def _seg_dist_sq(px, py, sx, sy, ex, ey):
    x, y = sx, sy
    dx, dy = ex - x, ey - y
    if dx != 0.0 or dy != 0.0:
        den = dx * dx + dy * dy
        num = (px - x) * dx + (py - y) * dy
        if den == 0.0:  # IEEE division, which Python refuses to do
            t = float("nan") if (num == 0.0 or num != num) else math.copysign(INF, num) * math.copysign(1.0, den)
        else:
            t = num / den
        if t > 1.0:
            x, y = ex, ey
        elif t > 0.0:
            x += dx * t
            y += dy * t
    dx, dy = px - x, py - y
    return dx * dx + dy * dy


def _div(a, b):
    if b == 0.0:
        if a == 0.0 or a != a:
            return float("nan")
        return math.copysign(INF, a) * math.copysign(1.0, b)
    return a / b


def point_dist(px, py, rings):
    inside = False
    m = INF
    for ring in rings:
        for i in range(1, len(ring)):
            ax, ay = ring[i]
            bx, by = ring[i - 1]
            if (ay > py) != (by > py) and px < _div((bx - ax) * (py - ay), (by - ay)) + ax:
                inside = not inside
            d = _seg_dist_sq(px, py, ax, ay, bx, by)
            assert d == d, "a NaN reached the distance minimum"
            if d < m:
                m = d
    return (1.0 if inside else -1.0) * math.sqrt(m)


def _area(ring):
    s = 0.0
    for i in range(1, len(ring)):
        s += ring[i][0] * ring[i - 1][1] - ring[i - 1][0] * ring[i][1]
    return abs(s)


def label_position(rings, scale, tie="std", capped=False):
    """-> (status, x, y, queue_peak, pops); rings: list of lists of (x, y)."""
    if not rings or not len(rings[0]):
        return NONE, 0.0, 0.0, 0, 0
    rings = [[(float(x), float(y)) for x, y in r] for r in rings]
    largest, largest_area = 0, _area(rings[0])
    for i in range(1, len(rings)):
        a = _area(rings[i])
        if a > largest_area:
            largest, largest_area = i, a
    lead = rings[largest]
    kept = [lead] + [r for i, r in enumerate(rings) if i != largest and all(point_dist(x, y, [lead]) >= 0.0 for x, y in r)]
    min_x = min_y = INF
    max_x = max_y = -INF
    for x, y in lead:
        min_x = x if x < min_x else min_x
        max_x = x if x > max_x else max_x
        min_y = y if y < min_y else min_y
        max_y = y if y > max_y else max_y
    w, h = max_x - min_x, max_y - min_y
    precision = (w if w > h else h) / 100.0 * scale
    cell_size = w if w < h else h
    max_size = w if w > h else h
    if cell_size == 0.0:
        return OK, min_x, min_y, 0, 0
    area = sx = sy = 0.0
    for i in range(1, len(lead)):
        ax, ay = lead[i]
        bx, by = lead[i - 1]
        c = ax * by - bx * ay
        sx += (ax + bx) * c
        sy += (ay + by) * c
        area += c * 3.0
    cen = lead[0] if area == 0.0 else (sx / area, sy / area)

    def fit(cx, cy, d):
        if d <= 0.0:
            return d
        dx, dy = cx - cen[0], cy - cen[1]
        return d * (1.0 - math.sqrt(dx * dx + dy * dy) / max_size)

    def cell(cx, cy, half):  # (max_fitness, fitness, cx, cy, half)
        d = point_dist(cx, cy, kept)
        c = (fit(cx, cy, d + half * SQRT_2), fit(cx, cy, d), cx, cy, half)
        assert c[0] == c[0] and c[1] == c[1], "a NaN reached a queue key"
        return c

    heap = _StdHeap() if tie == "std" else _OtherHeap()
    peak = pops = 0

    half = cell_size / 2.0
    x = min_x
    while x < max_x:
        y = min_y
        while y < max_y:
            if capped and len(heap) >= MAX_CELLS:
                return TOO_LARGE, 0.0, 0.0, peak, pops
            heap.push(cell(x + half, y + half, half))
            peak = max(peak, len(heap))
            y += cell_size
        x += cell_size
    best = cell(cen[0], cen[1], 0.0)
    while len(heap):
        if capped and pops >= MAX_CELLS:
            return TOO_LARGE, 0.0, 0.0, peak, pops
        cur = heap.pop()
        pops += 1
        if cur[1] > best[1]:
            best = cur
        if cur[0] - best[1] <= precision:
            continue
        half = cur[4] / 2.0
        for dx in (-1.0, 1.0):
            for dy in (-1.0, 1.0):
                if capped and len(heap) >= MAX_CELLS:
                    return TOO_LARGE, 0.0, 0.0, peak, pops
                heap.push(cell(cur[2] + dx * half, cur[3] + dy * half, half))
                peak = max(peak, len(heap))
    return OK, best[2], best[3], peak, pops


def bits(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


# ---- seeded request families (shared by the CPU and the GPU tests) ---------------------------------------------------
def star(rng, n=None):
    n = n or int(rng.integers(5, 14))
    cx, cy = rng.uniform(-50, 300, 2)
    r = rng.uniform(3, 80)
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    rad = r * rng.uniform(0.35, 1.0, n)
    p = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1)
    return np.concatenate([p, p[:1]])


def rot_rect(rng):
    cx, cy = rng.uniform(-50, 300, 2)
    a, b = rng.uniform(2, 90, 2)
    t = rng.uniform(0, np.pi)
    c, s = np.cos(t), np.sin(t)
    q = np.array([[-a, -b], [a, -b], [a, b], [-a, b], [-a, -b]]) / 2
    return np.stack([cx + q[:, 0] * c - q[:, 1] * s, cy + q[:, 0] * s + q[:, 1] * c], 1)


def l_shape(rng):
    x0, y0 = rng.uniform(-20, 200, 2)
    a, b = rng.uniform(10, 90, 2)
    t, u = rng.uniform(0.2, 0.8, 2)
    return np.array([[x0, y0], [x0 + a, y0], [x0 + a, y0 + b * u], [x0 + a * t, y0 + b * u], [x0 + a * t, y0 + b], [x0, y0 + b], [x0, y0]])


def u_shape(a, b, t):
    return np.array([[0, 0], [a, 0], [a, b], [a - t, b], [a - t, t], [t, t], [t, b], [0, b], [0, 0]], dtype=np.float64)


def plus_shape(a, t):
    m = (a - t) / 2
    return np.array([[m, 0], [m + t, 0], [m + t, m], [a, m], [a, m + t], [m + t, m + t], [m + t, a], [m, a], [m, m + t], [0, m + t], [0, m],
                     [m, m], [m, 0]], dtype=np.float64)


def square(a):
    return np.array([[0, 0], [a, 0], [a, a], [0, a], [0, 0]], dtype=np.float64)


def symmetric_family(rng, n):
    out = []
    for _ in range(n):
        k = int(rng.integers(0, 10))
        a = 2 * int(rng.integers(5, 60))
        if k < 7:
            out.append([u_shape(a, int(rng.integers(10, 120)), int(rng.integers(2, max(3, a // 2 - 1))))])
        elif k < 9:
            out.append([plus_shape(a, 2 * int(rng.integers(1, max(2, a // 2 - 1))))])
        else:
            out.append([square(a)])
    return out


def multipolygon(rng):
    outer = star(rng, int(rng.integers(6, 16)))
    c = outer[:-1].mean(0)
    rings = [outer]
    for _ in range(int(rng.integers(1, 4))):
        k = rng.uniform(0.05, 0.5)
        off = rng.uniform(-3, 3, 2)
        rings.append((c + off + (outer - c) * k)[::-1].copy())
    if rng.integers(0, 3) == 0:  # a ring outside the outer one
        rings.append(rot_rect(rng) + np.array([1000.0, 0.0]))
    if rng.integers(0, 4) == 0:  # the largest ring is not the first
        rings = rings[1:] + rings[:1]
    if rng.integers(0, 8) == 0:
        rings.insert(1, np.zeros((0, 2)))
    return rings


def seeded_requests(n, seed=1):
    """n requests: lists of rings (float64 [k, 2] arrays), drawn from all families in a fixed order."""
    rng = np.random.default_rng(seed)
    out = []
    sym = symmetric_family(rng, (n + 4) // 5)
    for i in range(n):
        k = i % 5
        if k == 0:
            out.append([star(rng)])
        elif k == 1:
            out.append([rot_rect(rng)])
        elif k == 2:
            out.append([l_shape(rng)])
        elif k == 3:
            out.append(sym[i // 5])
        else:
            out.append(multipolygon(rng))
    return out


def pack(requests, scales):
    """lists of rings -> (rings [n, 2] uint32, points [m, 2] float64, requests structured array) of the ABI."""
    from osm_renderer_amd import labels

    ring_rows, pts, n_pts = [], [], 0
    ring_off = np.zeros(len(requests), np.uint32)
    n_rings = np.zeros(len(requests), np.uint32)
    for i, rings in enumerate(requests):
        ring_off[i], n_rings[i] = len(ring_rows), len(rings)
        for r in rings:
            r = np.asarray(r, np.float64).reshape(-1, 2)
            ring_rows.append((n_pts, len(r)))
            pts.append(r)
            n_pts += len(r)
    req = np.zeros(len(requests), labels.LABEL_REQUEST_DTYPE)
    req["ring_off"], req["n_rings"], req["scale"] = ring_off, n_rings, scales
    rings_a = np.array(ring_rows, np.uint32).reshape(-1, 2)
    pts_a = np.concatenate(pts).astype(np.float64) if pts else np.zeros((0, 2))
    return rings_a, np.ascontiguousarray(pts_a.reshape(-1, 2)), req
