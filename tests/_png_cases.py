"""Named cases for the GPU PNG encoder (csrc/osmt_pngenc.hip), shared by tests/test_png_cases_cpu.py (what the model does on
them, no GPU) and tests/test_gpu_png_edges.py (the kernels against the model, byte for byte).

Most cases are written as a FILTERED stream — where the zeros, the bursts and the runs lie, row by row — and turned into the
image whose Paeth filter is exactly that stream (_png_model.unfilter; the round trip is asserted), so a case says directly
which decision of the matcher or of the run coder it is there for.  Notation as in _png_model: a row is f[0] = 4, f[1 .. 3W];
NB = 3W + 1; lane l owns the NBY = 3W / 64 bytes from L(l) = 1 + l * NBY; a band is H / 8 rows, r the row inside its band.
`events` are the keys of the model's trace (tile_tokens(..., trace=Counter())) the case must reach.  Everything is
deterministic: seeded generators, no state."""
import functools
from collections import Counter

import numpy as np

from tests import _png_model as M

FAST_SHAPES = [(8, 256), (16, 256), (72, 256), (8, 512), (64, 512), (16, 512), (256, 256)]
GENERIC_SHAPES = [(1, 4), (3, 8), (2, 20), (7, 256), (100, 256), (12, 512), (1024, 4), (9, 1020), (4, 1024)]
LMAX_LITERALS = [v for v in range(256) if M.LITLEN[v] == M.LMAX]  # the literals with the longest code
RUN_R = [2, 3, 258, 259, 260, 261, 516]  # R = L - 1: two literals, the shortest match, the cap and what follows it


class Case:
    def __init__(self, name, kind, img, events=()):
        self.name, self.kind, self.events = name, kind, tuple(events)
        self.img = np.ascontiguousarray(img, dtype=np.uint8)
        self.shape = self.img.shape[:2]  # (H, W)

    def __repr__(self):
        return "Case(%s %dx%d)" % ((self.name,) + self.shape)


def _rgba(rgb):
    out = np.full(rgb.shape[:2] + (4,), 255, dtype=np.uint8)
    out[..., :3] = rgb
    return out


class Stream:
    """the filtered bytes of an image, all zero until something is put; k counts as in the model (byte 0 is the filter type)"""

    def __init__(self, H, W):
        self.H, self.W, self.NB = H, W, 3 * W + 1
        self.NBY = 3 * W // 64
        self.rpb = H // M.LZ_BANDS
        self.F = np.zeros((H, self.NB), dtype=np.uint8)
        self.F[:, 0] = 4

    def L(self, lane):
        return 1 + lane * self.NBY

    def y(self, band, r):
        assert r < self.rpb
        return band * self.rpb + r

    def put(self, y, k, data):
        data = list(data)
        assert 1 <= k and k + len(data) <= self.NB, (k, len(data))
        assert not self.F[y, k : k + len(data)].any(), "two patterns overlap"
        self.F[y, k : k + len(data)] = data

    def image(self):
        rows = self.F[:, 1:]
        rgb = M.unfilter(rows, self.W)
        assert np.array_equal(M.paeth_filter(rgb), rows), "unfilter / paeth_filter round trip"
        return _rgba(rgb)


def pat(seed, n):
    """n non-zero bytes, no two neighbours equal (no zero: no burst inside; no run)"""
    v = np.random.default_rng(1000 + seed).integers(1, 256, size=n)
    for i in range(1, n):
        if v[i] == v[i - 1]:
            v[i] = v[i] % 255 + 1
    return [int(x) for x in v]


def other(b):
    """a non-zero byte that differs from b"""
    return (b ^ 0x80) or 0x7F


@functools.lru_cache(maxsize=None)
def colliding_words(shared):
    """two 4-byte words of non-zero bytes with one hash that agree on exactly `shared` leading bytes (0 or 2; 3 cannot be:
    the fourth byte is the top byte of the hashed word, and an odd multiplier moves the top byte of the product by a non-zero
    amount whenever only that byte changes — test_png_cases_cpu.py proves it over all 255 differences)"""
    rng = np.random.default_rng(77 + shared)
    seen = {}
    head = [int(x) for x in rng.integers(1, 256, size=shared)]
    while True:
        w = head + [int(x) for x in rng.integers(1, 256, size=4 - shared)]
        h = M.hash4(*w)
        for o in seen.get(h, ()):
            if o[shared] != w[shared]:
                return tuple(o), tuple(w)
        seen.setdefault(h, []).append(w)


def _pair(s, ys, ks, yd, kd, p, n, tail=True):
    """p at (ys, ks); at (yd, kd) its first n bytes and then a byte that differs from the source's"""
    s.put(ys, ks, p)
    s.put(yd, kd, p[:n] + ([other(p[n])] if tail and n < len(p) else []))


# ---------------------------------------------------------------------------------------------------------------------
# matcher cases: every band of a tile is a scenario of its own (a table and a history per band)
def matcher_a(H, W):
    s = Stream(H, W)
    NB, NBY, L, rpb = s.NB, s.NBY, s.L, s.rpb
    ev = []
    # band 0: hash collisions — a candidate that agrees on 0 bytes, one that agrees on 2
    (a0, b0), (a2, b2) = colliding_words(0), colliding_words(2)
    s.put(s.y(0, 0), L(1), list(a0) + pat(1, 3))
    s.put(s.y(0, 1), L(1), list(b0) + pat(2, 3))
    s.put(s.y(0, 0), L(5), list(a2) + pat(3, 3))
    s.put(s.y(0, 1), L(5), list(b2) + pat(4, 3))
    ev += [("agree", 0), ("declined_short", 2)]
    # band 1: the shortest matches, 4 and 5 bytes
    _pair(s, s.y(1, 0), L(1), s.y(1, 1), L(2), pat(5, 8), 4)
    _pair(s, s.y(1, 0), L(6), s.y(1, 1), L(5), pat(6, 8), 5)
    ev += [("taken_len", 4), ("taken_len", 5)]
    # band 2: the cap — 257 bytes agree; 300 bytes agree (258 are taken, the rest are literals)
    _pair(s, s.y(2, 0), L(0), s.y(2, 1), L(0), pat(7, 258), 257)
    far = L(24 if W == 256 else 14)
    _pair(s, s.y(2, 0), far, s.y(2, 1), far, pat(8, 300), 300)
    ev += [("taken_len", 257), ("taken_len", 258), "cap_beyond"]
    # band 3: distance 5 — the row's last four bytes, found again at byte 1 of the next row; the source row's end clamps the
    # match although the stream goes on alike (filter-type byte, then the same four bytes)
    p = pat(9, 4)
    s.put(s.y(3, 0), NB - 4, p)
    s.put(s.y(3, 1), 1, p + [4] + p)
    ev += [("dist", 5), "burst_at_row_end", "clamped_by_source_row"]
    # band 4: the largest distance — byte 1, found again seven rows down in the last four bytes
    if rpb >= 8:
        p = pat(10, 5)
        s.put(s.y(4, 0), 1, p)
        s.put(s.y(4, 7), NB - 4, p[:4])
        ev += [("dist", 8 * NB - 5), ("rows_up", 7), "ends_at_row_end"]
    # band 5: cover — a burst inside a taken match is declined; a burst exactly at its end is taken
    p = pat(11, NBY - 2) + [0, 0] + pat(12, 10)
    _pair(s, s.y(5, 0), L(2), s.y(5, 1), L(2), p + [9], len(p))
    q, b = pat(13, NBY - 1) + [0], pat(14, 9)
    s.put(s.y(5, 0), L(10), q + [other(b[0])])
    s.put(s.y(5, 0), L(20), b)
    s.put(s.y(5, 1), L(10), q + b[:8] + [other(b[8])])
    ev += ["covered_declined", "adjacent"]
    # band 6: where a match ends — inside a run, on the last and on the first byte of a lane's span; across three lanes
    p = pat(15, 6)
    s.put(s.y(6, 0), L(1), p + [33, 33, 99])
    s.put(s.y(6, 1), L(1), p + [33] * 5)
    _pair(s, s.y(6, 0), L(5), s.y(6, 1), L(5), pat(16, NBY + 1), NBY)
    _pair(s, s.y(6, 0), L(9), s.y(6, 1), L(9), pat(17, NBY + 2), NBY + 1)
    _pair(s, s.y(6, 0), L(13), s.y(6, 1), L(13), pat(18, 2 * NBY + 6), 2 * NBY + 5)
    ev += ["ends_inside_run", "ends_on_last_of_span", "ends_on_first_of_span", "spans_three_lanes"]
    # band 7: two bursts of one row with one hash — the later one is the candidate; a burst too close to the row's end
    p = pat(19, 6)
    s.put(s.y(7, 0), L(1), p + [21, 22])
    s.put(s.y(7, 0), L(5), p + [23, 24])
    s.put(s.y(7, 1), L(3), p + [21, 25])
    s.put(s.y(7, 1), NB - 3, [5, 6, 7])
    ev += ["same_hash_in_row", ("dist", NB + L(3) - L(5)), ("taken_len", 6), "burst_dropped"]
    return Case("matcher_a", "matcher", s.image(), ev)


def matcher_b(H, W):
    s = Stream(H, W)
    L, rpb = s.L, s.rpb
    ev = []
    # bands 0 | 1: one burst in the last row of a band and in the first row of the next — no match (a table per band); the
    # row after that finds it one row up
    p = pat(30, 8)
    s.put(s.y(0, rpb - 1), L(3), p)
    s.put(s.y(1, 0), L(3), p)
    s.put(s.y(1, 1), L(3), p)
    ev += ["stale_band_hit", ("rows_up", 1)]
    if rpb >= 8:  # band 4: seven rows up, mid-row
        _pair(s, s.y(4, 0), L(7), s.y(4, 7), L(9), pat(33, 9), 8)
        ev += [("rows_up", 7)]
    if rpb >= 9:
        # band 2: eight rows up — declined (the ring slot of row 0 now holds row 8 itself)
        p = pat(31, 8)
        s.put(s.y(2, 0), L(2), p)
        s.put(s.y(2, 8), L(2), p)
        # band 3: row 8 lies in the ring slot row 0 had; its match comes from row 3
        _pair(s, s.y(3, 3), L(2), s.y(3, 8), L(4), pat(32, 9), 8)
        ev += [("window_declined", 8), "taken_in_reused_ring_slot", ("rows_up", 5)]
    return Case("matcher_b", "matcher", s.image(), ev)


def _lanes_free(used, y, k, n, NBY):
    lanes = set(range((max(k - 1, 1) - 1) // NBY, (k + n - 1) // NBY + 1))  # the byte in front stays zero, the lane behind clean
    if lanes & used.setdefault(y, set()):
        return None
    return lanes


def len_ladder(H, W):
    """one hashed match per length symbol 1 .. 28 (the lengths 4 .. 258 that are a symbol's base)"""
    s = Stream(H, W)
    pairs = [(s.y(b, r), s.y(b, r + 1)) for r in range(0, s.rpb - 1, 2) for b in range(M.LZ_BANDS)]
    pi, k = 0, 1
    ev = []
    for i, n in enumerate(sorted(M.LEN_BASE[1:], reverse=True)):
        need = -(-(n + 2) // s.NBY) * s.NBY  # whole lanes: pattern, the byte that differs, a zero
        if k + need > s.NB:
            pi, k = pi + 1, 1
        _pair(s, pairs[pi][0], k, pairs[pi][1], k, pat(400 + i, n + 1), n)
        k += need
        ev.append(("len_sym", M._len_sym(n)))
    return Case("len_ladder", "matcher", s.image(), ev)


def dist_ladder(H, W):
    """one hashed match per distance symbol from 5 up to the largest the shape reaches (symbol 4 is distance 5 or 6: matcher_a):
    sources in row 0 of a band, the copies `up` rows below, k - k' chosen for the symbol"""
    s = Stream(H, W)
    NB, NBY = s.NB, s.NBY
    used = {}
    ev = []
    top = M._dist_sym(min(7, s.rpb - 1) * NB + NB - 5)
    for sym in range(5, top + 1):
        lo, hi = M.DIST_BASE[sym], M.DIST_BASE[sym + 1] - 1
        done = False
        for t in range(M.LZ_BANDS * 7):
            band, up = (sym + t) % M.LZ_BANDS, 1 + t // M.LZ_BANDS
            if up > s.rpb - 1 or done:
                continue
            ys, yd = s.y(band, 0), s.y(band, up)
            for d in (lo, (lo + hi) // 2, hi):
                dk = d - up * NB  # k - k'
                for ks in range(1, NB - 5):
                    kd = ks + dk
                    if not (1 <= kd <= NB - 5):
                        continue
                    ls, ld = _lanes_free(used, ys, ks, 5, NBY), _lanes_free(used, yd, kd, 5, NBY)
                    if ls is None or ld is None:
                        continue
                    used[ys] |= ls
                    used[yd] |= ld
                    _pair(s, ys, ks, yd, kd, pat(200 + sym, 5), 4)
                    done = True
                    break
                if done:
                    break
        assert done, "no place for distance symbol %d" % sym
        ev.append(("dist_sym", sym))
    return Case("dist_ladder", "matcher", s.image(), ev)


# ---------------------------------------------------------------------------------------------------------------------
# runs
def _ramp(n, start=0):
    return [200 + (start + i) % 50 for i in range(n)]  # literals, no two neighbours equal, apart from the run values below


def runs_rows(H, W):
    """filtered rows (H x NB): a row of one value; a row that starts with the filter-type byte's value and ends in a run over
    several lane spans; then runs of every length that matters, packed first-fit; what is left alternates zero / ramp rows"""
    NB = 3 * W + 1
    F = np.zeros((H, NB), dtype=np.uint8)
    F[:, 0] = 4
    F[0, 1:] = 7
    if H == 1:
        return F
    tail = min(100, (NB - 1) // 2)
    F[1, 1:] = ([4, 4, 4] + _ramp(NB))[: NB - 1]
    F[1, NB - tail :] = 9
    want = sorted({r + 1 for r in RUN_R + M.LEN_BASE}, reverse=True)
    bins = [[] for _ in range(2, H)]
    for n in want:
        for b in bins:
            if sum(b) + n <= NB - 1:
                b.append(n)
                break
    for i, b in enumerate(bins):
        y = 2 + i
        if not b:
            if i % 2:
                F[y, 1:] = _ramp(NB - 1, i)
            continue
        row = []
        for j, n in enumerate(b):
            row += [1 + (37 * (i * 16 + j)) % 199] * n
            if j and row[-n - 1] == row[-1]:
                row[-n:] = [row[-1] % 199 + 1] * n
        F[y, 1:] = (row + _ramp(NB))[: NB - 1]
    return F


def runs_case(H, W, kind="runs"):
    F = runs_rows(H, W)
    rgb = M.unfilter(F[:, 1:], W)
    assert np.array_equal(M.paeth_filter(rgb), F[:, 1:])
    ev = ["row_of_one_value"]
    if H >= 2 and W >= 8:
        ev += ["row_starts_with_filter_byte", "run_over_spans_to_row_end"]
    return Case("runs", kind, _rgba(rgb), ev)


# ---------------------------------------------------------------------------------------------------------------------
# size and checksums
def worst_rows(H, W, seed, rows=None):
    """every filtered byte of `rows` (default: all) a literal with the longest code, no two neighbours equal, no match: the rows
    of a band start with different bytes.  The other rows are zero."""
    NB = 3 * W + 1
    F = np.zeros((H, NB), dtype=np.uint8)
    F[:, 0] = 4
    n = len(LMAX_LITERALS)
    rng = np.random.default_rng(seed)
    for y in range(H) if rows is None else rows:
        idx = rng.integers(0, n, size=NB - 1)
        idx[0] = (y + seed) % n
        for i in range(1, NB - 1):
            if idx[i] == idx[i - 1]:
                idx[i] = (idx[i] + 1) % n
        F[y, 1:] = np.asarray(LMAX_LITERALS)[idx]
    return F


def _from_rows(name, kind, F, W, events=()):
    rgb = M.unfilter(F[:, 1:], W)
    assert np.array_equal(M.paeth_filter(rgb), F[:, 1:])
    return Case(name, kind, _rgba(rgb), events)


def worst_cases(H, W):
    out = [_from_rows("worst_0", "worst", worst_rows(H, W, 1), W), _from_rows("worst_1", "worst", worst_rows(H, W, 2), W)]
    if M.lz_applies(W, H):
        rpb = H // M.LZ_BANDS
        out.append(_from_rows("worst_band0_only", "worst_mixed", worst_rows(H, W, 3, rows=range(rpb)), W))
        out.append(_from_rows("worst_all_but_band0", "worst_mixed", worst_rows(H, W, 4, rows=range(rpb, H)), W))
    return out


def adler_ff(H, W):
    F = np.full((H, 3 * W + 1), 255, dtype=np.uint8)
    F[:, 0] = 4
    return _from_rows("adler_ff", "size", F, W)


def plain(H, W):
    """an image as the older tests draw them: flat ground, rectangles of flat colour, noise, gradients"""
    rng = np.random.default_rng(4242)
    im = np.zeros((H, W, 3), dtype=np.uint8)
    im[:] = rng.integers(0, 256, size=3)
    for _ in range(12):
        x0, y0 = rng.integers(0, W), rng.integers(0, H)
        w, h = rng.integers(1, W), rng.integers(1, H)
        sl = (slice(y0, min(H, y0 + h)), slice(x0, min(W, x0 + w)))
        kind = rng.integers(0, 3)
        if kind == 0:
            im[sl] = rng.integers(0, 256, size=3)
        elif kind == 1:
            im[sl] = rng.integers(0, 256, size=im[sl].shape)
        else:
            im[sl] = (np.arange(im[sl].shape[1])[None, :, None] * int(rng.integers(1, 9))) % 256
    return Case("plain", "plain", _rgba(im))


def noise(H, W):
    return Case("noise", "generic", _rgba(np.random.default_rng(H * 4099 + W).integers(0, 256, size=(H, W, 3))))


def flat(H, W, colour=(241, 238, 232), name="flat"):
    im = np.zeros((H, W, 3), dtype=np.uint8)
    im[:] = colour
    return Case(name, "size" if name == "black" else "generic", _rgba(im))


@functools.lru_cache(maxsize=None)
def by_shape():
    """{(H, W): [cases]} — the cases of one shape go through the encoder in ONE call"""
    out = {}
    for H, W in FAST_SHAPES:
        cs = out.setdefault((H, W), [])
        if (H, W) == (256, 256):
            cs.append(plain(H, W))
            continue
        if (H, W) != (16, 512):
            if H // M.LZ_BANDS >= 2:
                cs += [matcher_a(H, W), matcher_b(H, W), len_ladder(H, W), dist_ladder(H, W)]
            else:  # one row per band: no history, no row to fetch ahead
                cs += [noise(H, W), flat(H, W)]
            cs.append(runs_case(H, W))
        if (H, W) in ((8, 256), (16, 512)):
            cs += worst_cases(H, W)
        if (H, W) in ((72, 256), (64, 512)):
            cs.append(adler_ff(H, W))
        if (H, W) == (8, 256):
            cs.append(flat(H, W, (0, 0, 0), "black"))
    for H, W in GENERIC_SHAPES:
        cs = out.setdefault((H, W), [])
        cs += [noise(H, W), flat(H, W), runs_case(H, W, "generic")]
        if (H, W) == (4, 1024):
            cs += worst_cases(H, W)
        if (H, W) == (9, 1020):
            cs.append(adler_ff(H, W))
        if (H, W) == (1, 4):
            cs.append(flat(H, W, (0, 0, 0), "black"))
    return out


def all_cases():
    return [c for cs in by_shape().values() for c in cs]


@functools.lru_cache(maxsize=None)
def _model(shape, name, lz):
    c = next(c for c in by_shape()[shape] if c.name == name)
    return M.encode(c.img, lz=lz)


def model_file(case, lz=None):
    """the model's file of a case (computed once per process)"""
    return _model(case.shape, case.name, lz)


@functools.lru_cache(maxsize=None)
def _trace(shape, name):
    c = next(c for c in by_shape()[shape] if c.name == name)
    t = Counter()
    toks, _ = M.tile_tokens(c.img, trace=t)
    return t, toks


def trace(case):
    """(the model's trace of a case, its tokens)"""
    return _trace(case.shape, case.name)
