"""What a k_raster wave does before it draws: the early exit of the blocks past the batch, the job record taken as words
(canvas bytes, n_ops), the list header beside it, the first chunk's staging loads and the constants a stroke visit reads.

Every case is compared bit for bit with the oracle (RGBA8 on every tile, the f64 canvas on some).  Batches of at most 64
tiles take the FOLD instantiation (the waves read the op bits themselves), bigger ones the list path (k_sublist's
headers), so the shapes that matter run both ways: alone and as the first tile of 65."""
import numpy as np
import pytest

from osm_renderer_amd import abi, display_list
from osm_renderer_amd.display_list import TileBuilder
from tests._parity import assert_parity

pytestmark = pytest.mark.gpu
CAPS = [abi.CAP_NONE, abi.CAP_BUTT, abi.CAP_ROUND, abi.CAP_SQUARE]
# the sub-tile (32 x 16 pixels, times the scale) the shaped tiles put their ops into: column 2, row 3
SX, SY = 2, 3


def _mixed_tile(rnd, n_ops, scale=1, canvas=(241, 238, 232)):
    tb = TileBuilder(scale=scale, canvas=canvas)
    W = 256 * scale
    for i in range(n_ops):
        p = rnd.integers(0, W, size=2)
        if i % 3 == 0:
            r = int(rnd.integers(4, 50)) * scale
            tb.fill([(p[0] - r, p[1] - r), (p[0] + r, p[1] - r // 2), (p[0] + r // 3, p[1] + r), (p[0] - r, p[1] - r)],
                    tuple(rnd.integers(0, 256, size=3)), float(rnd.choice([1.0, 0.5])))
        elif i % 3 == 1:
            pts = (p + np.cumsum(rnd.integers(-40, 41, size=(3, 2)) * scale, axis=0)).tolist()
            tb.stroke(pts, float(rnd.choice([1.0, 2.5, 6.0])) * scale, tuple(rnd.integers(0, 256, size=3)), float(rnd.choice([1.0, 0.7])),
                      cap=CAPS[i % 4])
        else:
            q = p + rnd.integers(-80, 81, size=2) * scale
            tb.stroke([p.tolist(), q.tolist()], 3.0 * scale, tuple(rnd.integers(0, 256, size=3)), 0.8, dashes=[7.0, 4.0], cap=CAPS[(i + 1) % 4])
    return tb.build()


def _in_batch_of_65(tile):
    """The tile in front of 64 tiles of plain canvas: more than OSMT_FOLD_MAX_JOBS tiles, so it gets lists."""
    rest = [TileBuilder(canvas=(i, 255 - i, 7 * i % 256)).build() for i in range(64)]
    return display_list.concat([tile] + rest)


def _both_ways(gpu_ctx, oracle, tile, msg):
    assert_parity(gpu_ctx, oracle, tile, f64_jobs=[0], msg=msg + ", alone (fold)")
    assert_parity(gpu_ctx, oracle, _in_batch_of_65(tile), f64_jobs=[0], msg=msg + ", first of 65 (lists)")


# ---- early exit: the grid is a whole number of groups of eight tiles ----------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 9, 70])
def test_batches_that_do_not_fill_their_last_group_of_eight(gpu_ctx, oracle, n):
    rnd = np.random.default_rng(100 + n)
    dl = display_list.concat([_mixed_tile(rnd, int(rnd.integers(1, 9)), canvas=(3 * i % 256, 200, 255 - i)) for i in range(n)])
    assert_parity(gpu_ctx, oracle, dl, f64_jobs=sorted({0, n - 1}), msg=f"{n} tiles")


# ---- the canvas bytes, taken from the words of the job record -------------------------------------------------------------
CANVASES = [None, (0, 1, 127), (128, 254, 255), (255, 0, 128), (1, 255, 254), (127, 128, 0), None, (254, 127, 1)]


@pytest.mark.parametrize("n", [8, 72])
def test_canvas_bytes_and_tiles_without_a_canvas(gpu_ctx, oracle, n):
    rnd = np.random.default_rng(7)
    tiles = [_mixed_tile(rnd, 3, canvas=CANVASES[i % len(CANVASES)]) for i in range(n)]
    dl = display_list.concat(tiles)
    got = assert_parity(gpu_ctx, oracle, dl, f64_jobs=[0, 1, 2, 3, 4, 5], msg=f"canvas bytes, {n} tiles")
    assert (got[..., 3] == 255).all()


@pytest.mark.parametrize("n", [5, 66])
def test_one_tile_without_ops_among_tiles_with_ops(gpu_ctx, oracle, n):
    rnd = np.random.default_rng(11)
    tiles = [_mixed_tile(rnd, 0 if i == n // 2 else 4, canvas=(10 + i, 128, 255)) for i in range(n)]
    dl = display_list.concat(tiles)
    got = assert_parity(gpu_ctx, oracle, dl, f64_jobs=[n // 2], msg=f"one empty tile of {n}")
    assert (got[n // 2] == np.array([10 + n // 2, 128, 255, 255], dtype=np.uint8)).all()


@pytest.mark.parametrize("n", [5, 67])
def test_all_tiles_without_ops(gpu_ctx, oracle, n):
    tiles = [TileBuilder(canvas=None if i % 4 == 3 else (i, 255 - i, 128)).build() for i in range(n)]
    dl = display_list.concat(tiles)
    got = assert_parity(gpu_ctx, oracle, dl, f64_jobs=[0, n - 1], msg=f"{n} tiles, no op at all")
    assert (got[3, ..., :3] == 0).all(), "no canvas: opaque black"


# ---- scales: nsub = 128 and 1152 (not a power of two) -------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1, 3])
def test_nine_tiles_of_a_dozen_ops(gpu_ctx, oracle, scale):
    rnd = np.random.default_rng(40 + scale)
    dl = display_list.concat([_mixed_tile(rnd, 12, scale=scale, canvas=(255 - 20 * i, 17 * i, 128)) for i in range(9)])
    assert_parity(gpu_ctx, oracle, dl, f64_jobs=[0, 8], msg=f"nine tiles at scale {scale}")


# ---- shapes of the first chunk of one sub-tile ------------------------------------------------------------------------------------
def _fill(tb, k, scale=1):
    x0, y0 = (32 * SX + 2 + k % 7) * scale, (16 * SY + 1 + k % 3) * scale
    tb.fill([(x0, y0), (x0 + (12 + k) * scale, y0 + 2 * scale), (x0 + 5 * scale, y0 + (9 + k % 4) * scale), (x0, y0)],
            (40 * k % 256, (255 - 30 * k) % 256, 90 + k), 1.0 if k % 2 else 0.6)


def _stroke(tb, k, scale=1, **kw):
    x0, y0 = (32 * SX + 1 + 2 * (k % 9)) * scale, (16 * SY + 2 + k % 5) * scale
    tb.stroke([(x0, y0), (x0 + (9 + k % 6) * scale, y0 + (4 + k % 7) * scale), (x0 + 20 * scale, y0 - 1 * scale)],
              kw.pop("width", 1.5 + 0.5 * (k % 4)) * scale, ((255 - 25 * k) % 256, (60 + 11 * k) % 256, 20 * k % 256), 0.9 if k % 3 else 1.0, **kw)


def _long_stroke(tb):
    """One op with far more than 256 slots (every edge's window is most of the tile) that crosses the sub-tile."""
    pts = []
    for i in range(24):
        pts.append((4 + 10 * i, 2 if i % 2 == 0 else 250))
    pts.append((32 * SX + 16, 16 * SY + 8))
    tb.stroke(pts, 3.0, (200, 30, 90), 0.8, cap=abi.CAP_ROUND)


def _shape(name):
    tb = TileBuilder(canvas=(250, 248, 240))
    if name == "only_fills":
        for k in range(9):
            _fill(tb, k)
    elif name == "only_strokes":
        for k in range(9):
            _stroke(tb, k, cap=CAPS[k % 4])
    elif name == "sixteen_stroke_first_and_last":
        _stroke(tb, 0)
        for k in range(1, 15):
            _fill(tb, k) if k % 3 else _stroke(tb, k)
        _stroke(tb, 15, cap=abi.CAP_SQUARE)
    elif name == "big_first_stroke":
        _long_stroke(tb)
        for k in range(5):
            _fill(tb, k) if k % 2 else _stroke(tb, k)
    elif name == "seventeen_entries":
        for k in range(17):
            _fill(tb, k) if k % 2 else _stroke(tb, k, cap=CAPS[k % 4])
    elif name == "stroke_kinds":
        _stroke(tb, 1)                                                             # un-dashed
        _stroke(tb, 2, width=3.0, dashes=[5.0, 3.0])                               # dashed, the fast path
        _stroke(tb, 3, width=3.0, dashes=[4.0, 2.0, 1.0, 2.0], cap=abi.CAP_ROUND, use_caps_for_dashes=True)  # original endpoints
        _stroke(tb, 4, width=5.0, cap=abi.CAP_ROUND)                               # cap stubs
        _stroke(tb, 5, width=4.0, cap=abi.CAP_SQUARE, dashes=[6.0, 6.0])
        _fill(tb, 3)
    elif name == "twenty_strokes":
        for k in range(20):
            _stroke(tb, k, dashes=[3.0 + k % 3, 2.0] if k % 4 == 1 else None, cap=CAPS[k % 4])
    return tb.build()


@pytest.mark.parametrize("name", ["only_fills", "only_strokes", "sixteen_stroke_first_and_last", "big_first_stroke", "seventeen_entries",
                                  "stroke_kinds", "twenty_strokes"])
def test_first_chunk_shapes(gpu_ctx, oracle, name):
    _both_ways(gpu_ctx, oracle, _shape(name), name)
