"""The case corpus of the GPU PNG encoder (tests/_png_cases.py) on the CPU: the model's files of all cases decode to their
images; every case reaches, by the model's trace, the decisions it was built for; the corpus as a whole covers every length and
distance symbol the matcher can produce; the worst-case tiles cost exactly what the slot bound assumes; and a model that deviates
from the specification in one rule of the matcher writes a different file for at least one case — so a kernel that deviated in
that way fails the byte comparison of tests/test_gpu_png_edges.py.  No GPU."""
import io
import zlib
from collections import Counter

import numpy as np
import pytest

from tests import _png_cases as C
from tests import _png_model as M

# One rule of the matcher changed at a time (keys of _png_model.RULES).
MUTANTS = {
    "min_match_2": dict(min_match=2),
    "min_match_3": dict(min_match=3),
    "min_match_5": dict(min_match=5),
    "window_6": dict(window=6),
    "window_8": dict(window=8),
    "cap_257": dict(cap=257),
    "cover_strict": dict(cover_strict=True),      # `k > cover` in place of `k >= cover`
    "burst_strict": dict(burst_strict=True),      # `k + 4 < NB` in place of `k + 4 <= NB`
    "no_table_reset": dict(reset_tables=False),   # one table and one history for the whole tile
    "insert_first": dict(insert_first=True),      # a row's bursts enter the table before the row looks them up
    "keep_earliest": dict(keep_earliest=True),    # the earliest burst of a hash stays in its slot, not the latest
}
# min_match 2 and 3: a candidate never agrees on exactly 3 bytes (test_no_candidate_agrees_on_exactly_three_bytes), so 3 is
# the specification under another name; 2 is not, and a candidate that agrees on exactly 2 bytes is in the corpus.
EQUIVALENT = {"min_match_3"}


def _cases(kind=None):
    return [c for c in C.all_cases() if kind is None or c.kind == kind]


def _ids(cases):
    return ["%s-%dx%d" % ((c.name,) + c.shape) for c in cases]


def test_unfilter_inverts_the_paeth_filter():
    rng = np.random.default_rng(11)
    for H, W in ((1, 4), (5, 7), (16, 64), (3, 300)):
        rows = rng.integers(0, 256, size=(H, 3 * W), dtype=np.uint8)
        img = M.unfilter(rows, W)
        assert img.shape == (H, W, 3) and img.dtype == np.uint8
        assert np.array_equal(M.paeth_filter(img), rows)
        rgb = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        assert np.array_equal(M.unfilter(M.paeth_filter(rgb), W), rgb)


def test_trace_and_rules_leave_the_model_alone():
    """with a trace, and with the rules passed explicitly, the tokens are those of the plain call"""
    for c in _cases("matcher")[:4] + _cases("runs")[:2]:
        plain = M.tile_tokens(c.img)[0]
        assert M.tile_tokens(c.img, trace=Counter())[0] == plain
        assert M.tile_tokens(c.img, rules=dict(M.RULES))[0] == plain


@pytest.mark.parametrize("case", _cases(), ids=_ids(_cases()))
def test_model_file_decodes_to_the_image(case):
    from PIL import Image

    png = C.model_file(case)
    H, W = case.shape
    assert np.array_equal(np.array(Image.open(io.BytesIO(png)).convert("RGB")), case.img[..., :3])
    idat_len = int.from_bytes(png[33:37], "big")
    raw = zlib.decompress(png[41 : 41 + idat_len])
    want = np.concatenate([np.full((H, 1), 4, dtype=np.uint8), M.paeth_filter(case.img[..., :3])], axis=1)
    assert raw == want.tobytes()
    assert np.array_equal(M.unfilter(np.frombuffer(raw, dtype=np.uint8).reshape(H, 3 * W + 1)[:, 1:], W), case.img[..., :3])


@pytest.mark.parametrize("case", _cases(), ids=_ids(_cases()))
def test_case_reaches_its_events(case):
    tr, toks = C.trace(case)
    missing = [e for e in case.events if not tr[e]]
    assert not missing, "%r does not reach %s" % (case, missing)
    if not M.lz_applies(case.shape[1], case.shape[0]):
        assert all(t[0] == "lit" or t[2] == 1 for t in toks), "the generic kernel codes runs only"


def _corpus_trace(pred):
    tot = Counter()
    for c in _cases():
        if pred(c):
            tot.update(C.trace(c)[0])
    return tot


def _syms(tr, key):
    return {k[1] for k in tr if isinstance(k, tuple) and k[0] == key}


@pytest.mark.parametrize("W,top", [(256, 25), (512, 27)])
def test_symbol_coverage_of_the_matcher(W, top):
    tr = _corpus_trace(lambda c: c.shape[1] == W and M.lz_applies(W, c.shape[0]))
    assert _syms(tr, "len_sym") == set(range(1, 29)), "hashed matches: every length symbol but 0 (length 3 is below the minimum)"
    assert _syms(tr, "dist_sym") >= set(range(4, top + 1))
    assert max(_syms(tr, "dist")) == 8 * (3 * W + 1) - 5 and min(_syms(tr, "dist")) == 5
    assert max(_syms(tr, "dist_sym")) == top
    # the threshold from both sides, and the collisions
    assert tr["agree", 0] and tr["declined_short", 2] and tr["taken_len", 4] and tr["taken_len", 5]
    assert not tr["agree", 3]


def test_rows_per_band_of_the_corpus():
    tr = _corpus_trace(lambda c: True)
    assert _syms(tr, "rows_per_band") == {1, 2, 8, 9, 32}
    assert tr["window_declined", 8] and tr["taken_in_reused_ring_slot"] and tr["stale_band_hit"]


@pytest.mark.parametrize("shape", [(8, 256), (8, 512), (9, 1020)])
def test_run_lengths_and_run_symbols(shape):
    """one row per band (no hashed match interferes) and one generic width: every run length that matters, every length symbol"""
    case = next(c for c in C.by_shape()[shape] if c.name == "runs")
    tr, toks = C.trace(case)
    assert all(t[0] == "lit" or t[2] == 1 for t in toks)
    assert _syms(tr, "run_R") >= set(C.RUN_R) | set(M.LEN_BASE)
    assert _syms(tr, "run_sym") == set(range(29))
    assert tr["row_of_one_value"] and tr["row_starts_with_filter_byte"] and tr["run_over_spans_to_row_end"]


@pytest.mark.parametrize("case", _cases("worst") + _cases("worst_mixed"), ids=_ids(_cases("worst") + _cases("worst_mixed")))
def test_worst_case_tiles_cost_the_bound(case):
    """every filtered byte of the worst rows is a literal of lmax bits: rows * (len(lit 4) + 3W * lmax) bits per band — 8 * 7 bits
    below 12 bits per filtered byte at 8 x 256 (73 768 of 73 824), which sizes band_cap_words, the staging offsets and
    osmt_png_device_bound"""
    H, W = case.shape
    toks, rows = M.tile_tokens(case.img)
    assert all(t[0] == "lit" for t in toks) or case.kind == "worst_mixed"
    worst = [y for y in range(H) if rows[y][1] in C.LMAX_LITERALS]
    per_row = M.LITLEN[4] + 3 * W * M.LMAX
    i = 0
    for y in range(H):  # the tokens of row y: from one literal 4 at a row's start to the next
        j = i + 1
        n = 1
        while n < 3 * W + 1:
            n += 1 if toks[j][0] == "lit" else toks[j][1]
            j += 1
        bits = sum(M._tok_bits(t) for t in toks[i:j])
        if y in worst:
            assert bits == per_row and all(t[0] == "lit" for t in toks[i:j]), "row %d" % y
            assert all(rows[y][k] != rows[y][k + 1] for k in range(3 * W))
        else:
            assert bits < 128, "a zero row is three or six run matches"
        i = j
    assert i == len(toks)
    if case.kind == "worst":
        assert len(worst) == H
        assert sum(M._tok_bits(t) for t in toks) == H * per_row
        if (H, W) == (8, 256):
            assert H * per_row == 73768
        if (H, W) == (16, 512):
            assert H * per_row == 294992
    else:
        rpb = H // M.LZ_BANDS
        assert worst in (list(range(rpb)), list(range(rpb, H)))
    assert H * per_row <= H * (3 * W + 1) * M.LMAX


def test_smallest_files_are_shorter_than_the_crc_has_threads():
    """the CRC of the IDAT chunk is dealt to 512 threads (fast kernel) or 256 (generic): fewer bytes than threads"""
    for shape, threads in (((8, 256), 512), ((1, 4), 256)):
        case = next(c for c in C.by_shape()[shape] if c.name == "black")
        png = C.model_file(case)
        assert len(png) - 37 - 16 < threads, len(png)  # "IDAT" + data: the file without its first 37 and last 16 bytes


def test_no_candidate_agrees_on_exactly_three_bytes():
    """the fourth byte of a burst is the top byte of the hashed word: changing it alone moves the top byte of the product by
    d * 2654435761 mod 256, which is non-zero for every d in 1 .. 255 (the multiplier is odd) — the hash, the product's top
    eight bits, changes.  Two bursts of one hash that share three bytes share the fourth: the threshold `n >= 4` can be missed
    from below only by a collision that agrees on 0, 1 or 2 bytes, and a minimum of 3 is the same matcher as a minimum of 4."""
    assert all((d * 2654435761) & 0xFF for d in range(1, 256))
    rng = np.random.default_rng(5)
    for b0, b1, b2 in rng.integers(0, 256, size=(64, 3)):
        assert len({M.hash4(int(b0), int(b1), int(b2), b3) for b3 in range(256)}) == 256


@pytest.mark.parametrize("name", list(MUTANTS))
def test_the_corpus_tells_a_deviating_matcher_from_the_model(name):
    rules = dict(M.RULES, **MUTANTS[name])
    told = None
    for c in _cases("matcher"):
        if M.tile_tokens(c.img, rules=rules)[0] != C.trace(c)[1]:
            told = c
            break
    if name in EQUIVALENT:
        assert told is None, "%s is told apart by %r: three agreeing bytes were thought impossible" % (name, told)
        return
    assert told is not None, "no case tells %s from the specification" % name
    if all(t[0] == "lit" or t[1] >= 3 for t in M.tile_tokens(told.img, rules=rules)[0]):  # (deflate has no code for a match of 2)
        assert M.encode(told.img, rules=rules) != C.model_file(told)
