"""Byte-exact CPU model of the GPU PNG encoder (csrc/osmt_pngenc.hip): ONE deflate block under the constant prefix codes of
tests/golden/png_huffman.json (literal/length and distance), Paeth filter, distance-1 runs and — on the kernel's fast path,
256- or 512-pixel-wide images whose height splits into eight bands — LZ77 matches found through a small hash table per band
(round 6).  Test infrastructure for tests/test_gpu_png_device.py; the model IS the specification of the kernel's choices:

  row            f[0] = 4 (Paeth), f[1 .. 3W] the filtered bytes; NB = 3W + 1
  lane           l = 0 .. 63 owns the bytes [1 + l * NBY, 1 + (l + 1) * NBY), NBY = 3W / 64
  burst          the FIRST byte k of a lane's span with f[k] != 0 and (k == 1 or f[k - 1] == 0), if k + 4 <= NB
  hash           ((f[k] | f[k+1] << 8 | f[k+2] << 16 | f[k+3] << 24) * 2654435761 mod 2^32) >> 24: 256 slots per band, holding
                 1 + (row in band << 11 | k) of the LATEST burst with that hash (rows above only: a row inserts its bursts
                 after it has looked its own up)
  candidate      the slot's burst, if it lies at most 7 rows above (the kernel keeps a ring of eight rows in LDS) and at least
                 4 bytes agree; the match runs to the first differing byte, at most 258 bytes, and stays inside both rows;
                 distance = rows * NB + k - k'
  selection      lanes in order: a candidate is taken if it starts at or behind the end of the last taken one
  tokens         the bytes outside the taken matches are coded as before (literal, distance-1 matches of <= 258 for the rest
                 of a run, <= 2 trailing literals), a run ending where a taken match or the row ends

The matcher's rules are the entries of RULES; row_matches / tile_tokens / encode take `rules` (a deviation, for the sensitivity
test of tests/test_png_cases_cpu.py) and row_matches / tile_tokens a `trace` (a Counter of what the matcher and the run coder
met).  With neither, the output is that of the rules above.  unfilter() is the inverse of paeth_filter: tests/_png_cases.py
writes its cases as filtered streams.

The canonical codes are derived here from the code lengths (RFC 1951 3.2.2); the block header bits come with the lengths
(they describe them: any inflater — zlib, PIL in the tests — checks that the two agree)."""
import json, os, struct, zlib
import numpy as np

LEN_BASE = [3,4,5,6,7,8,9,10,11,13,15,17,19,23,27,31,35,43,51,59,67,83,99,115,131,163,195,227,258]
LEN_EXTRA = [0,0,0,0,0,0,0,0,1,1,1,1,2,2,2,2,3,3,3,3,4,4,4,4,5,5,5,5,0]
DIST_BASE = [1,2,3,4,5,7,9,13,17,25,33,49,65,97,129,193,257,385,513,769,1025,1537,2049,3073,4097,6145,8193,12289,16385,24577]
DIST_EXTRA = [0,0,0,0,1,1,2,2,3,3,4,4,5,5,6,6,7,7,8,8,9,9,10,10,11,11,12,12,13,13]
LZ_HASH_BITS = 8
LZ_MIN_MATCH = 4
LZ_WINDOW_ROWS = 7
LZ_BANDS = 8  # row bands of a tile (PNG_BANDS: the waves of the kernel's workgroup), each with a table and a history of its own

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_huffman.json")) as _f:
    _T = json.load(_f)
LITLEN = _T["litlen_lengths"]
DISTLEN = _T["dist_lengths"] if len(_T["dist_lengths"]) == 30 else [5] * 30  # (a table from before round 6: the generator is about to replace it)
LMAX = _T["lmax"]
HDR_BITS, HDR_N = int(_T["block_header_hex"], 16), _T["block_header_bits"]
TOKENS_BIT = 43 * 8 + HDR_N           # PNG_TOKENS_BIT: file bit the first token starts at
HEAD_WORDS = (24 + HDR_N + 31) // 32  # PNG_HEAD_WORDS

def rev(code, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (code & 1); code >>= 1
    return r

def _canonical(lengths):
    maxl = max(lengths)
    count = [0] * (maxl + 1)
    for l in lengths:
        if l: count[l] += 1
    code = 0; nxt = [0] * (maxl + 2)
    for bits in range(1, maxl + 1):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for l in lengths:
        out.append(nxt[l] if l else 0)
        if l: nxt[l] += 1
    return out

CODES = _canonical(LITLEN)
DCODES = _canonical(DISTLEN)

def lit_token(v):
    return rev(CODES[v], LITLEN[v]), LITLEN[v]

def dist_token(d):
    idx = max(i for i in range(30) if DIST_BASE[i] <= d)
    eb = DIST_EXTRA[idx]; ev = d - DIST_BASE[idx]
    hb, hn = rev(DCODES[idx], DISTLEN[idx]), DISTLEN[idx]
    return hb | (ev << hn), hn + eb

def len_token(L, d=1):
    """length code + extra bits, then the distance code + extra bits"""
    idx = max(i for i in range(29) if LEN_BASE[i] <= L)
    s = 257 + idx; eb = LEN_EXTRA[idx]; ev = L - LEN_BASE[idx]
    hb, hn = rev(CODES[s], LITLEN[s]), LITLEN[s]
    db, dn = dist_token(d)
    return hb | (ev << hn) | (db << (hn + eb)), hn + eb + dn

def paeth_filter(rgb):
    H, W, _ = rgb.shape
    raw = rgb.reshape(H, W * 3).astype(np.int32)
    a = np.zeros_like(raw); a[:, 3:] = raw[:, :-3]
    b = np.zeros_like(raw); b[1:] = raw[:-1]
    c = np.zeros_like(raw); c[1:, 3:] = raw[:-1, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return ((raw - pred) & 255).astype(np.uint8)

class Bits:
    """LSB-first bit stream; whole bytes leave the accumulator every 4096 bits (one growing integer made a 1024-wide tile quadratic)"""
    def __init__(self): self.acc = 0; self.n = 0; self.done = []
    def put(self, v, nb):
        self.acc |= v << self.n; self.n += nb
        if self.n >= 4096:
            k = self.n // 8
            self.done.append((self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, 'little'))
            self.acc >>= 8 * k; self.n -= 8 * k
    def bytes(self):
        nb = (self.n + 7) // 8
        return b''.join(self.done) + self.acc.to_bytes(nb, 'little')

def lz_applies(W, H):
    """the kernel's fast path (k_png_encode_fast): the only one that searches for matches"""
    return W in (256, 512) and H % LZ_BANDS == 0 and H >= LZ_BANDS

def hash4(b0, b1, b2, b3):
    w = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24)
    return ((w * 2654435761) & 0xFFFFFFFF) >> (32 - LZ_HASH_BITS)

RULES = dict(min_match=LZ_MIN_MATCH, window=LZ_WINDOW_ROWS, cap=258, cover_strict=False, burst_strict=False, reset_tables=True,
             insert_first=False, keep_earliest=False)
"""the matcher's rules as parameters: the defaults ARE the specification; tests/test_png_cases_cpu.py passes deviations
(`rules=dict(RULES, min_match=5)`, ...) to show that the case corpus tells each of them from the specification"""

def _len_sym(L):
    return max(i for i in range(29) if LEN_BASE[i] <= L)

def _dist_sym(d):
    return max(i for i in range(30) if DIST_BASE[i] <= d)

def row_bursts(row, NB, NBY, strict=False, trace=None):
    """the first burst of every lane's span (see above); trace: 'burst_at_row_end' (k + 4 == NB), 'burst_dropped' (k + 4 > NB)"""
    bursts = []
    for l in range(64):
        s0 = 1 + l * NBY
        for k in range(s0, s0 + NBY):
            if row[k] != 0 and (k == 1 or row[k - 1] == 0):
                if (k + 4 < NB) if strict else (k + 4 <= NB):
                    bursts.append(k)
                    if trace is not None and k + 4 == NB: trace['burst_at_row_end'] += 1
                elif trace is not None:
                    trace['burst_dropped'] += 1
                break
    return bursts

def row_matches(row, NB, NBY, r, table, hist, trace=None, rules=None):
    """the matches the kernel takes in one row (list of (k, length, distance)), then the row's own insertions.
    trace (a collections.Counter) counts what the matcher met — see the keys below; without it nothing is recorded and
    the result is the same."""
    R = RULES if rules is None else rules
    bursts = row_bursts(row, NB, NBY, R['burst_strict'], trace)
    hs = [hash4(row[k], row[k + 1], row[k + 2], row[k + 3]) for k in bursts]
    if trace is not None and len(set(hs)) < len(hs):
        trace['same_hash_in_row'] += 1
    def insert():
        for k, h in zip(bursts, hs):
            v = 1 + ((r << 11) | k)
            if R['keep_earliest']:
                table[h] = table[h] or v
            else:
                table[h] = max(table[h], v)
    if R['insert_first']:
        insert()
    taken = []
    cover = 0
    for k, h in zip(bursts, hs):
        v = table[h]
        if not v:
            continue
        cr, ck = (v - 1) >> 11, (v - 1) & 2047
        if r - cr > R['window']:
            if trace is not None: trace['window_declined', r - cr] += 1
            continue
        d = (r - cr) * NB + (k - ck)
        if d <= 0:  # (insert_first only: the row's own entry)
            continue
        src = hist[cr] if cr < len(hist) else row
        mx = min(R['cap'], NB - k, NB - ck)
        n = 0
        while n < mx and src[ck + n] == row[k + n]:
            n += 1
        if trace is not None:
            trace['agree', min(n, 6)] += 1  # bytes a candidate agrees on: 0 .. 5 exactly, 6 = more
            if n < R['min_match']: trace['declined_short', n] += 1
        if n >= R['min_match'] and (k > cover if R['cover_strict'] else k >= cover):
            if trace is not None:
                trace['taken_len', n] += 1
                trace['len_sym', _len_sym(n)] += 1
                trace['dist', d] += 1
                trace['dist_sym', _dist_sym(d)] += 1
                trace['rows_up', r - cr] += 1
                if r >= 8: trace['taken_in_reused_ring_slot'] += 1
                if n == R['cap'] and k + n < NB and ck + n < NB and src[ck + n] == row[k + n]: trace['cap_beyond'] += 1
                if k + n == NB: trace['ends_at_row_end'] += 1
                if n == NB - ck and n < min(R['cap'], NB - k): trace['clamped_by_source_row'] += 1
                if cover and k == cover: trace['adjacent'] += 1
                if k + n < NB and row[k + n] == row[k + n - 1]: trace['ends_inside_run'] += 1
                if (k + n - 1) % NBY == 0: trace['ends_on_last_of_span'] += 1
                if (k + n - 1) % NBY == 1: trace['ends_on_first_of_span'] += 1
                if (k + n - 2) // NBY - (k - 1) // NBY >= 2: trace['spans_three_lanes'] += 1
            taken.append((k, n, d))
            cover = k + n
        elif trace is not None and n >= R['min_match']:
            trace['covered_declined'] += 1
    if not R['insert_first']:
        insert()
    return taken

def _stale_hits(row, NB, NBY, table, hist, rpb):
    """trace only: bursts of a band's first row that the table of the band ABOVE would have matched (>= 4 bytes) in that
    band's last row — what a kernel that did not start every band from an empty table would take"""
    hits = 0
    for k in row_bursts(row, NB, NBY):
        v = table[hash4(row[k], row[k + 1], row[k + 2], row[k + 3])]
        if v and (v - 1) >> 11 == rpb - 1:
            ck = (v - 1) & 2047
            n = 0
            while n < min(NB - k, NB - ck) and hist[rpb - 1][ck + n] == row[k + n]: n += 1
            hits += n >= LZ_MIN_MATCH
    return hits

def tile_tokens(rgba, lz=None, trace=None, rules=None):
    """(tokens, filtered rows): ('lit', v) and ('match', length, distance) in stream order.
    trace keys — matcher: ('agree', n) ('declined_short', n) ('taken_len', n) ('len_sym', s) ('dist', d) ('dist_sym', s)
    ('rows_up', rows) ('window_declined', rows) 'taken_in_reused_ring_slot' 'cap_beyond' 'ends_at_row_end'
    'clamped_by_source_row' 'adjacent' 'covered_declined' 'ends_inside_run' 'ends_on_last_of_span' 'ends_on_first_of_span'
    'spans_three_lanes' 'same_hash_in_row' 'burst_at_row_end' 'burst_dropped' 'stale_band_hit' ('rows_per_band', n);
    runs: ('run_R', R) for R = L - 1 >= 2, ('run_sym', s) per distance-1 match, 'row_of_one_value', 'run_over_spans_to_row_end',
    'row_starts_with_filter_byte'"""
    R_ = RULES if rules is None else rules
    H, W, _ = rgba.shape
    f = paeth_filter(rgba[..., :3])
    NB = 3 * W + 1
    use_lz = lz_applies(W, H) if lz is None else lz
    rows = [bytes([4]) + f[y].tobytes() for y in range(H)]
    out = []
    span = (NB - 1 + 63) // 64  # a lane's bytes (both kernels)
    if use_lz:
        NBY = 3 * W // 64
        rpb = H // LZ_BANDS
        if trace is not None: trace['rows_per_band', rpb] += 1
        table = None
    for y in range(H):
        row = rows[y]
        taken = []
        if use_lz:
            b, r = divmod(y, rpb)
            if not R_['reset_tables']:
                r = y
            if r == 0:
                if trace is not None and table is not None and _stale_hits(row, NB, NBY, table, hist, rpb):
                    trace['stale_band_hit'] += 1
                table = [0] * (1 << LZ_HASH_BITS)
                hist = []
            taken = row_matches(row, NB, NBY, r, table, hist, trace, rules)
            hist.append(row)
        if trace is not None:
            if row[1] == 4: trace['row_starts_with_filter_byte'] += 1
            if row[1] != 0 and row[1:] == row[1:2] * (NB - 1): trace['row_of_one_value'] += 1
        row_toks = [('lit', 4)]
        i = 1; ti = 0
        while i < NB:
            if ti < len(taken) and taken[ti][0] == i:
                row_toks.append(('match', taken[ti][1], taken[ti][2]))
                i += taken[ti][1]; ti += 1
                continue
            v = row[i]
            seg_end = taken[ti][0] if ti < len(taken) else NB
            j = i + 1
            while j < seg_end and row[j] == v: j += 1
            row_toks.append(('lit', v))
            R = j - i - 1
            if trace is not None and R >= 2:
                trace['run_R', R] += 1
                if j == NB and (j - 2) // span > (i - 1) // span and i > 1: trace['run_over_spans_to_row_end'] += 1
            while R >= 3:
                m = min(R, 258); row_toks.append(('match', m, 1)); R -= m
                if trace is not None: trace['run_sym', _len_sym(m)] += 1
            row_toks += [('lit', v)] * R
            i = j
        out += row_toks
    return out, rows

def unfilter(rows, W):
    """the inverse of paeth_filter: rows = H x 3W filtered bytes -> the H x W x 3 image whose paeth_filter is exactly `rows`.
    Plain integers; a pixel needs its left, upper and upper-left neighbours, so the anti-diagonals are done one after another."""
    rows = np.asarray(rows, dtype=np.uint8)
    H = rows.shape[0]
    assert rows.shape == (H, 3 * W)
    f = rows.reshape(H, W, 3).astype(np.int32)
    img = np.zeros((H + 1, W + 1, 3), dtype=np.int32)  # row 0 and column 0: the zeros outside the image
    for d in range(H + W - 1):
        ys = np.arange(max(0, d - W + 1), min(H, d + 1))
        xs = d - ys
        a, b, c = img[ys + 1, xs], img[ys, xs + 1], img[ys, xs]
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        img[ys + 1, xs + 1] = (f[ys, xs] + pred) & 255
    return img[1:, 1:].astype(np.uint8)

def _tok_bits(t):
    return lit_token(t[1])[1] if t[0] == 'lit' else len_token(t[1], t[2])[1]

def encode(rgba, lz=None, rules=None):
    H, W, _ = rgba.shape
    toks, rows = tile_tokens(rgba, lz=lz, rules=rules)
    bw = Bits(); bw.put(HDR_BITS, HDR_N)
    for t in toks:
        if t[0] == 'lit':
            b, n = lit_token(t[1])
        else:
            b, n = len_token(t[1], t[2])
        bw.put(b, n)
    A, B = 1, 0
    for row in rows:
        stream = np.frombuffer(row, dtype=np.uint8).astype(np.int64)
        nn = len(stream)
        B = (B + nn * A + int(((nn - np.arange(nn)) * stream).sum())) % 65521
        A = (A + int(stream.sum())) % 65521
    t, tn = lit_token(256); bw.put(t, tn)
    deflate = bw.bytes()
    idat = b'\x78\x01' + deflate + struct.pack('>I', (B << 16) | A)
    def chunk(t, d): return struct.pack('>I', len(d)) + t + d + struct.pack('>I', zlib.crc32(t + d) & 0xFFFFFFFF)
    return b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 2, 0, 0, 0)) + chunk(b'IDAT', idat) + chunk(b'IEND', b'')
