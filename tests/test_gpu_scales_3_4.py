"""Scales 3 and 4 end to end, GPU against the oracle bit for bit.  Above scale 2 the code changes shape: 24 x 48 = 1152
sub-tiles at scale 3 (no power of two), 32 x 64 = 2048 at scale 4, where the per-row sub-tile mask is full (bit 31 live),
`fill_geom` packs ncols = 32 and nsr = 64 and k_sublist's offset table is exactly full.

Paths the tests of this file take, and what selects them (stated as assertions on the display lists below):
  * fold — a batch of at most 64 tiles whose tiles have at most 128 ops: k_raster<FOLD> builds the lists (1 tile, ~30 ops);
  * k_sublist, small batch — a tile of more than 128 ops rendered alone;
  * k_sublist, one cursor — 65 tiles (more than 64: lists for every tile; fewer than 128: one cursor);
  * k_sublist, sixteen cursors and the overflow slice — 130 tiles (>= OSMT_LIST_SLICE_MIN_JOBS = 128); the long tile sits at
    indices 5 and 5 + 32 (both cursor 5) and its lists alone exceed a slice of the entry arena, so it and the later tiles of
    its slice are placed in the overflow slice;
  * RGB8 output at scale 3 (rows of 2304 bytes), the host-buffer entry with a pinned output (chunks of 128 / scale^2 = 14
    and 8 tiles, n = 2 chunks + 3, the last chunk partial) and a pageable one, twice on a fresh context so that the second
    call sizes its arenas from the density the first one measured at that scale;
  * the refusal of scenes of 2^28 fill groups and more (OSMT_MAX_FILL_GROUPS), which only scale 4 brings within reach."""
import numpy as np
import pytest

from osm_renderer_amd import abi, display_list
from osm_renderer_amd.display_list import JOB_DTYPE, OP_DTYPE, RING_DTYPE, DisplayList, TileBuilder
from tests._parity import assert_parity

pytestmark = pytest.mark.gpu

SCALES = [3, 4]
CAPS = [abi.CAP_NONE, abi.CAP_BUTT, abi.CAP_ROUND, abi.CAP_SQUARE]
SUB_W, SUB_H = 32, 16  # OSMT_SUB_W, OSMT_SUB_H
FOLD_MAX_OPS, FOLD_MAX_JOBS, SLICE_MIN_JOBS, LIST_SLICES = 128, 64, 128, 16
CANVAS_EDGE = (250, 246, 235)


def _col(rnd):
    return tuple(int(v) for v in rnd.integers(0, 256, size=3))


def _box(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)]


def corner_and_border_dots(scale):
    """(x, y) of a two-pixel fill in each corner sub-tile and in the middle sub-tile of each border"""
    W = 256 * scale
    m = W // 2 + 3
    return [(1, 2), (W - 3, 2), (1, W - 2), (W - 3, W - 2), (m, 2), (m, W - 2), (1, m), (W - 3, m)]


def edge_tile(scale):
    """The grid-edge tile: every op touches the first or last sub-tile column or row.  Translucent colours that differ
    from op to op, so that an entry out of place or out of order shows."""
    W = 256 * scale
    rnd = np.random.default_rng(3400 + scale)
    tb = TileBuilder(x=1, scale=scale, canvas=CANVAS_EDGE)
    op = lambda: (_col(rnd), float(rnd.choice([0.8, 0.55, 0.3])))
    for x, y in corner_and_border_dots(scale):  # pixels x, x + 1 of row y
        tb.fill(_box(x, y - 1, x + 1, y), *op())
    tb.fill(_box(W - SUB_W - 8, W // 3, W - SUB_W + 8, W // 3 + 40), *op())  # across the last column boundary
    tb.fill(_box(W // 3, W - SUB_H - 4, W // 3 + 70, W - SUB_H + 4), *op())  # across the last row boundary
    tb.fill(_box(W - SUB_W - 8, W - SUB_H - 4, W - SUB_W + 8, W - SUB_H + 4), *op())  # across both
    tb.fill(_box(-5, -5, W + 5, W + 5), *op())  # the window is clipped on all four sides: every sub-tile
    tb.fill(_box(-5, -5, W - SUB_W - 1, W + 5), *op())  # all but the last column
    tb.fill(_box(-5, -5, W + 5, W - SUB_H - 1), *op())  # all but the last row
    tb.stroke([(W - 1, -9), (W - 1, W + 9)], 1.0 * scale, *op())  # along x = W - 1
    tb.stroke([(-9, W - 1), (W + 9, W - 1)], 1.0 * scale, *op(), dashes=[7.0 * scale, 3.0 * scale])  # along y = W - 1
    # centre lines outside the tile by 3 px, half-width 3: only the feather reaches column 0 / nsx - 1, row 0 / sub_rows - 1
    tb.stroke([(-3, -20), (-3, W + 20)], 6.0, *op())
    tb.stroke([(W + 2, W + 20), (W + 2, -20)], 6.0, *op())
    tb.stroke([(-20, -3), (W + 20, -3)], 6.0, *op(), cap=abi.CAP_SQUARE)
    tb.stroke([(W + 20, W + 2), (-20, W + 2)], 6.0, *op(), dashes=[9.0, 4.0])
    # the same a little further out (4 px: nothing reaches the tile) and a little nearer (2 px)
    tb.stroke([(-4, -20), (-4, W + 20)], 6.0, *op())
    tb.stroke([(W + 1, -20), (W + 1, W + 20)], 6.0, *op())
    # a dashed stroke with round caps that ends inside the last column
    tb.stroke([(W // 2, W // 3), (W - 40, W // 3 + 5), (W - 9, W // 3 + 11)], 3.0 * scale, *op(), dashes=[5.0 * scale, 3.0 * scale],
              cap=abi.CAP_ROUND, use_caps_for_dashes=True)
    tb.stroke([(W - 20, W - 60), (W - 6, W - 7)], 2.0 * scale, *op(), dashes=[4.0 * scale, 2.0 * scale], cap=abi.CAP_ROUND)
    return tb.build()


def many_ops_tile(scale, n_ops=170):
    """more than 128 small ops all over the tile, the far columns and rows included: its lists come from k_sublist in any batch"""
    W = 256 * scale
    rnd = np.random.default_rng(3500 + scale)
    tb = TileBuilder(x=2, scale=scale, canvas=_col(rnd))
    for k in range(n_ops):
        far = k % 3 == 0  # a third of the ops in the last two columns / rows
        cx = int(rnd.integers(W - 2 * SUB_W, W + 4)) if far else int(rnd.integers(-4, W))
        cy = int(rnd.integers(W - 2 * SUB_H, W + 4)) if far and k % 2 else int(rnd.integers(-4, W))
        if k % 4 == 3:
            tb.nop()
        elif k % 2:
            pts = (np.array([cx, cy]) + np.cumsum(rnd.integers(-25 * scale, 25 * scale + 1, size=(3, 2)), axis=0)).tolist()
            tb.stroke([(cx, cy)] + pts, float(rnd.choice([1.0, 2.5, 5.0])) * scale, _col(rnd), float(rnd.choice([1.0, 0.6])),
                      dashes=[6.0 * scale, 3.0 * scale] if k % 5 == 0 else None, cap=CAPS[k % 4])
        else:
            r = int(rnd.integers(3, 30 * scale))
            tb.fill([(cx - r, cy - r), (cx + r, cy - r // 3), (cx + r // 2, cy + r), (cx - r, cy + r // 2), (cx - r, cy - r)], _col(rnd),
                    float(rnd.choice([1.0, 0.7, 0.35])))
    return tb.build()


LONG_POLYGONS = 150


def long_tile(scale):
    """150 polygons that each contain the square [40 s, 215 s]^2, and strokes across them"""
    s = scale
    rnd = np.random.default_rng(3600 + scale)
    tb = TileBuilder(x=3, scale=scale, canvas=(200, 210, 220))
    for k in range(LONG_POLYGONS):
        x0, y0 = (int(v) for v in rnd.integers(-5, 36 * s, size=2))
        x1, y1 = (int(v) for v in rnd.integers(219 * s, 262 * s, size=2))
        tb.fill([(x0, y0), (x1, y0 + 3), (x1 - 4, y1), (x0 + 2, y1 - 5), (x0, y0)], _col(rnd), float(rnd.choice([1.0, 0.2, 0.05])))
        if k % 10 == 0:
            tb.stroke([(0, (5 + k) * s), (256 * s, (250 - k) * s)], 3.0 * s, _col(rnd), 0.7)
    return tb.build()


def empty_tile(scale):
    return TileBuilder(x=4, scale=scale, canvas=(9, 8, 7)).build()


def list_entries_upper_bound(dl):
    """No more list entries than this: one per sub-tile of every fill's bounding box and of every stroke segment's, both
    grown by the stroke's reach and two pixels and clipped to the tile.  (The arenas the library sizes are no larger.)"""
    W = dl.dim
    total = 0
    for j in dl.jobs:
        for o in dl.ops[j["op_off"]: j["op_off"] + j["n_ops"]]:
            if o["kind"] == abi.OP_NONE:
                continue
            reach = 2 + (abs(float(o["width"])) / 2 + 1 if o["kind"] == abi.OP_STROKE else 0)
            for r in dl.rings[o["ring_off"]: o["ring_off"] + o["n_rings"]]:
                p = dl.coords[r["first_pt"]: r["first_pt"] + r["n_pts"]].astype(np.int64)
                boxes = [(p.min(0), p.max(0))] if o["kind"] != abi.OP_STROKE else [(np.minimum(a, b), np.maximum(a, b)) for a, b in zip(p[:-1], p[1:])]
                for lo, hi in boxes:
                    x0, y0 = np.clip(np.floor(lo - reach), 0, W - 1).astype(int)
                    x1, y1 = np.clip(np.ceil(hi + reach), 0, W - 1).astype(int)
                    if hi[0] + reach < 0 or hi[1] + reach < 0 or lo[0] - reach > W - 1 or lo[1] - reach > W - 1:
                        continue
                    # (a stroke's boxes count twice: its cap stubs are segments of their own beside the first and last edge)
                    total += (x1 // SUB_W - x0 // SUB_W + 1) * (y1 // SUB_H - y0 // SUB_H + 1) * (2 if o["kind"] == abi.OP_STROKE else 1)
    return total


class Pool:
    """the distinct tiles of one scale and their oracle framebuffers, rendered once"""

    EDGE, MANY, LONG, EMPTY = 0, 1, 2, 3

    def __init__(self, oracle, scale):
        self.scale = scale
        self.dls = [edge_tile(scale), many_ops_tile(scale), long_tile(scale), empty_tile(scale)]
        self.refs = oracle.render_batch(display_list.concat(self.dls), images=(), threads=4)
        self._dev = None

    def batch(self, idx):
        return display_list.concat([self.dls[i] for i in idx])

    def refs_on_device(self, device):
        import torch

        if self._dev is None:
            self._dev = torch.from_numpy(self.refs).to(device)
        return self._dev


_POOLS = {}


@pytest.fixture(scope="module")
def pools(oracle):
    def get(scale):
        if scale not in _POOLS:
            _POOLS[scale] = Pool(oracle, scale)
        return _POOLS[scale]

    yield get
    _POOLS.clear()


def layout(n):
    """n pool indices: empty tiles first, in the middle and last; the long tile at 5 and 5 + 32 (with sixteen cursors: the
    same cursor twice); the edge tile and the tile of many ops in turn everywhere else"""
    idx = [Pool.EDGE if k % 2 else Pool.MANY for k in range(n)]
    for k in (0, 1, n // 2, n // 2 + 1, n - 2, n - 1):
        idx[k] = Pool.EMPTY
    idx[5] = idx[5 + 32] = Pool.LONG
    return idx


def _same(got, want, msg):
    bad = np.nonzero((got != want).any(axis=-1))
    assert len(bad[0]) == 0, (f"{msg}: {len(bad[0])} pixels differ; first (tile,y,x)={tuple(int(b[0]) for b in bad)} "
                              f"gpu={got[bad][0].tolist()} oracle={want[bad][0].tolist()}")


# ---- the grid's edges and both list builders ------------------------------------------------------------------------------


@pytest.mark.parametrize("scale", SCALES)
def test_edge_tile_draws_where_it_claims(oracle, pools, scale):
    """(oracle only) the inputs are not vacuous: the tiny fills colour their corner and border sub-tiles, the strokes whose
    centre lines lie 3 px outside reach the outermost pixel rows and columns, the ones 4 px outside were the last to matter"""
    pool, W = pools(scale), 256 * scale
    ref = pool.refs[Pool.EDGE]
    dl = pool.dls[Pool.EDGE]
    only = lambda keep: DisplayList(_jobs_with(dl, len(keep)), dl.ops[keep], dl.rings, dl.coords, dl.dashes, dl.coord_kind, dl.scale)
    kinds = dl.ops["kind"]
    first_feather = int(np.nonzero(kinds == abi.OP_STROKE)[0][2])
    parts = oracle.render_batch(display_list.concat([only(list(range(8)))] + [only([first_feather + k]) for k in range(6)]), threads=7)
    dots, sides = parts[0], parts[1:]
    for x, y in corner_and_border_dots(scale):
        assert (dots[y, x, :3] != np.array(CANVAS_EDGE)).any(), (x, y)
        assert (dots[y, x] == dots[y, x + 1]).all()
    assert ((dots[..., :3] != np.array(CANVAS_EDGE)).any(-1)).sum() == 16
    changed = [(s[..., :3] != np.array(CANVAS_EDGE)).any(-1) for s in sides]
    assert changed[0][:, 0].all() and not changed[0][:, 1:].any()  # x = -3: column 0 only
    assert changed[1][:, W - 1].all() and not changed[1][:, : W - 1].any()
    assert changed[2][0, :].all() and not changed[2][1:, :].any()
    assert changed[3][W - 1, :].any() and not changed[3][: W - 1, :].any()
    assert not changed[4].any()  # x = -4: half-width 3 + feather does not reach pixel 0
    assert changed[5][:, W - 2:].all() and not changed[5][:, : W - 2].any()
    assert len(np.unique(np.ascontiguousarray(ref).view(np.uint32))) > 40


def _jobs_with(dl, n_ops):
    j = dl.jobs.copy()
    j["n_ops"] = n_ops
    return j


@pytest.mark.parametrize("scale", SCALES)
def test_edge_tile_alone_lists_folded(gpu_ctx, oracle, pools, scale):
    pool = pools(scale)
    dl = pool.dls[Pool.EDGE]
    assert dl.n_jobs == 1 <= FOLD_MAX_JOBS and 0 < len(dl.ops) <= FOLD_MAX_OPS and dl.dim == 256 * scale
    got = assert_parity(gpu_ctx, oracle, dl, msg=f"edge tile, scale {scale}")
    _same(got, pool.refs[[Pool.EDGE]], "edge tile against the pool")


@pytest.mark.parametrize("scale", SCALES)
def test_tiles_of_many_ops_alone_lists_from_k_sublist(gpu_ctx, oracle, pools, scale):
    pool = pools(scale)
    for which in (Pool.MANY, Pool.LONG):
        dl = pool.dls[which]
        assert dl.n_jobs == 1 and len(dl.ops) > FOLD_MAX_OPS
        scene = gpu_ctx.upload(dl)
        assert scene.max_tile_ops() == len(dl.ops)
        scene.free()
        got = assert_parity(gpu_ctx, oracle, dl, msg=f"tile {which} alone, scale {scale}")
        _same(got, pool.refs[[which]], "against the pool")


@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("scale", SCALES)
def test_batches_with_lists_for_every_tile(gpu_ctx, pools, scale, n):
    import torch

    pool = pools(scale)
    idx = layout(n)
    dl = pool.batch(idx)
    nsub = (dl.dim // SUB_W) * (dl.dim // SUB_H)
    assert nsub == {3: 1152, 4: 2048}[scale]
    assert dl.n_jobs == n > FOLD_MAX_JOBS  # k_sublist builds every tile's lists
    assert (n >= SLICE_MIN_JOBS) == (n == 130)  # 65: one cursor; 130: sixteen
    per_tile = dl.jobs["n_ops"]
    assert per_tile[0] == per_tile[1] == per_tile[n // 2] == per_tile[n - 1] == 0  # empty tiles first, in the middle, last
    assert per_tile[5] == per_tile[37] == len(pool.dls[Pool.LONG].ops) > LONG_POLYGONS and 5 % LIST_SLICES == 37 % LIST_SLICES
    assert (per_tile[2:5] > 0).all() and per_tile.max() > FOLD_MAX_OPS
    if n >= SLICE_MIN_JOBS:
        # the long tile's lists exceed a slice: its polygons all draw into every sub-tile inside [40 s, 215 s]^2, and a slice
        # holds a sixteenth of the batch's entries
        inside = (215 * scale // SUB_W - -(-40 * scale // SUB_W)) * (215 * scale // SUB_H - -(-40 * scale // SUB_H))
        slice_cap = -(-(list_entries_upper_bound(dl) + 1) // LIST_SLICES)
        assert LONG_POLYGONS * inside > slice_cap, (LONG_POLYGONS * inside, slice_cap)
    scene = gpu_ctx.upload(dl)
    got = gpu_ctx.render(scene)
    want = pool.refs_on_device(got.device)
    pick = torch.as_tensor(idx, device=got.device)
    bad_tiles = torch.nonzero((got != want[pick]).flatten(1).any(1)).flatten().cpu().tolist()
    if bad_tiles:  # the first differing tile, in full
        t = bad_tiles[0]
        _same(got[t:t + 1].cpu().numpy(), pool.refs[[idx[t]]], f"{n} tiles at scale {scale}: tiles {bad_tiles[:10]} differ; tile {t} (pool {idx[t]})")
    scene.free()


# ---- the operation classes of test_gpu_parity_ops.py with content in the far columns and rows -----------------------------


@pytest.mark.parametrize("scale", SCALES)
def test_fills_random_polygons(gpu_ctx, oracle, scale):
    rnd = np.random.default_rng(1234 + scale)
    W = 256 * scale
    tiles = []
    for t in range(3):
        tb = TileBuilder(scale=scale, canvas=_col(rnd))
        for k in range(25):
            n = int(rnd.integers(3, 12))
            c = rnd.integers(-40 * scale, W + 40, size=2)
            if k % 3 == 0:
                c = rnd.integers(W - 70, W + 40, size=2)  # around the far corner
            pts = (c + rnd.integers(-70 * scale, 70 * scale + 1, size=(n, 2))).tolist()  # self-intersecting, any winding
            if rnd.random() < 0.8:
                pts.append(pts[0])
            tb.fill(pts, _col(rnd), float(rnd.choice([1.0, 0.7, 0.33, 0.05])))
        tiles.append(tb.build())
    assert_parity(gpu_ctx, oracle, display_list.concat(tiles), msg=f"random fills scale {scale}")


@pytest.mark.parametrize("scale", SCALES)
def test_strokes_all_caps_dashes_widths(gpu_ctx, oracle, scale):
    """the generator of test_gpu_parity_ops.test_strokes_all_caps_dashes_widths; every other stroke starts in the last 64 pixels"""
    rnd = np.random.default_rng(77 + scale)
    dash_sets = [None, [3, 3], [10, 8], [6, 6], [1, 2, 3], [0.5, 0.5], [12, 3, 2, 3], [4]]
    widths = [0.0, 0.1, 0.5, 1.0, 1.5, 2.0, 3.0, 4.5, 7.0, 15.0]
    tiles = []
    W = 256 * scale
    for t in range(6):
        tb = TileBuilder(scale=scale, canvas=(252, 248, 228))
        for k in range(14):
            n = int(rnd.integers(2, 7))
            p0 = rnd.integers(-20, W + 20, size=2) if k % 2 else rnd.integers(W - 64, W + 20, size=2)
            pts = (p0 + np.cumsum(rnd.integers(-60 * scale, 60 * scale + 1, size=(n, 2)), axis=0)).tolist()
            d = dash_sets[int(rnd.integers(0, len(dash_sets)))]
            tb.stroke(pts, float(widths[int(rnd.integers(0, len(widths)))]) * scale, _col(rnd), float(rnd.choice([1.0, 0.6, 0.3])),
                      dashes=None if d is None else [v * scale for v in d], cap=CAPS[int(rnd.integers(0, 4))],
                      use_caps_for_dashes=bool(rnd.integers(0, 2)))
        tiles.append(tb.build())
    assert_parity(gpu_ctx, oracle, display_list.concat(tiles), msg=f"strokes scale {scale}")


@pytest.mark.parametrize("scale", SCALES)
def test_long_way_and_multipolygon_cross_the_tile_on_the_block_path(gpu_ctx, oracle, scale):
    """one way and one multi-ring polygon of more than 64 edges, from outside the tile on one side to outside on the other"""
    s, W = scale, 256 * scale
    wave = [(int(x), int(W - 40 * s + 38 * s * np.sin(x / (17.0 * s)))) for x in range(-100 * s, W + 100 * s, 3 * s)]  # along the last rows
    ring_a = [(int(W / 2 + 140 * s * np.cos(a)), int(W / 2 + 125 * s * np.sin(a))) for a in np.linspace(0, 2 * np.pi, 150)]  # past all four edges
    ring_b = [(int(W / 2 + 60 * s * np.cos(a)), int(W / 2 - 8 * s + 55 * s * np.sin(-a))) for a in np.linspace(0, 2 * np.pi, 90)]
    ring_c = [(int(W - 10 * s + 90 * s * np.cos(a)), int(40 * s + 80 * s * np.sin(a))) for a in np.linspace(0, 2 * np.pi, 70)]  # over the last columns
    for r in (ring_a, ring_b, ring_c):
        r[-1] = r[0]
    assert len(wave) - 1 > 64 and len(ring_a) + len(ring_b) + len(ring_c) - 3 > 64
    tb = TileBuilder(scale=scale)
    tb.stroke(wave, 6.0 * s, (30, 30, 200), 0.6, dashes=[7.0 * s, 4.0 * s], cap=abi.CAP_ROUND, use_caps_for_dashes=True)
    tb.fill([ring_a, ring_b, ring_c], (20, 160, 60), 0.7)
    tb.stroke(ring_a, 1.0 * s, (0, 0, 0), 1.0)
    assert_parity(gpu_ctx, oracle, tb.build(), msg=f"long ops scale {scale}")


@pytest.mark.parametrize("scale", SCALES)
def test_fill_many_crossings_in_the_last_column_band(gpu_ctx, oracle, scale):
    """the comb of test_fill_many_crossings_uses_the_streaming_path, scaled, and its dense part (160 crossings per row) moved
    into the last 32-pixel column band and the last three sub-tile rows.  The dense part is 44 rows tall whatever the scale:
    a row beyond the buffers of the fill pre-pass is streamed by one lane, 20 ms a row (the 210 rows of the scale-1 test
    take 4.3 s a render, 840 rows at scale 4 took 17 s)."""
    s, W = scale, 256 * scale
    pts = []
    for i in range(60):
        x = (2 + 4 * i) * s
        pts += [(x, 10 * s), (x + s, 200 * s), (x + 2 * s, 10 * s)]
    pts += [(250 * s, 5 * s), (2 * s, 5 * s), (2 * s, 10 * s)]
    tb = TileBuilder(scale=scale)
    tb.fill(pts, (10, 10, 200), 0.7)
    dense = []
    for i in range(80):
        x = W - SUB_W + (i * 31) % 32
        dense += [(x, W - 48 + (i % 7)), (x + (i % 3) - 1, W - 4 - (i % 11))]
    dense.append(dense[0])
    assert min(p[0] for p in dense) >= W - SUB_W - 1 and min(p[1] for p in dense) >= W - 3 * SUB_H and len(dense) - 1 > 128  # FILL_EMAX
    tb.fill(dense, (200, 10, 10), 0.6)
    assert_parity(gpu_ctx, oracle, tb.build(), msg=f"comb scale {scale}")


@pytest.mark.parametrize("scale", SCALES)
def test_image_fill_at_large_coordinates(gpu_ctx, oracle, scale):
    """Filler::Image looks its pixel up at (x % w, y % h): a 7 x 5 icon (no power of two) and a 16 x 16 one over x >= 768 or
    the tile's last columns"""
    rnd = np.random.default_rng(5 + scale)
    icon = rnd.integers(0, 256, size=(7, 5, 4), dtype=np.uint8)
    icon[0, 0, 3] = 0
    icon[1, 1, 3] = 255
    icon2 = rnd.integers(0, 256, size=(16, 16, 4), dtype=np.uint8)
    ids = [gpu_ctx.register_image(icon), gpu_ctx.register_image(icon2)]
    images = [np.zeros((1, 1, 4), np.uint8)] * ids[0] + [icon, icon2]
    s, W = scale, 256 * scale
    x_far = min(768, W - 2 * SUB_W)
    tb = TileBuilder(scale=scale)
    tb.fill([(10 * s, 10 * s), (250 * s, 40 * s), (200 * s, 250 * s), (30 * s, 200 * s), (10 * s, 10 * s)], (0, 0, 0), 1.0)
    tb.fill_image([(50 * s, 50 * s), (W + 9, 90 * s), (W - 3, 220 * s), (60 * s, 200 * s), (50 * s, 50 * s)], ids[0], opacity=0.3)
    tb.fill_image(_box(x_far, W // 2, W + 30, W + 30), ids[1])
    assert_parity(gpu_ctx, oracle, tb.build(), images=images, msg=f"image fill scale {scale}")


# ---- outputs ------------------------------------------------------------------------------------------------------------


def test_rgb8_rows_of_2304_bytes(gpu_ctx, pools):
    pool = pools(3)
    idx = [Pool.EDGE, Pool.MANY, Pool.EMPTY, Pool.LONG, Pool.EDGE]
    dl = pool.batch(idx)
    assert dl.dim * 3 == 2304
    got = gpu_ctx.render_batch_rgb(dl).reshape(len(idx), dl.dim, dl.dim, 3)
    _same(got, pool.refs[idx][..., :3], "RGB8 at scale 3")


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
@pytest.mark.parametrize("scale", SCALES)
def test_host_buffer_entry_twice_on_a_fresh_context(pools, scale, pinned):
    from osm_renderer_amd.renderer import Context

    pool = pools(scale)
    chunk = 128 // (scale * scale)
    assert chunk == {3: 14, 4: 8}[scale]
    n = 2 * chunk + 3  # the pinned pipeline needs 2 chunks; the third is partial
    idx = [(Pool.EDGE, Pool.MANY, Pool.EMPTY)[k % 3] for k in range(n)]
    idx[4] = Pool.LONG
    dl = pool.batch(idx)
    assert dl.n_jobs == n == {3: 31, 4: 19}[scale] and n % chunk == 3
    # sized on the device, and so measured for density[scale], not taken at the worst case: the worst case passes 32 MiB
    n_fills = int(np.isin(dl.ops["kind"], (abi.OP_FILL_COLOR, abi.OP_FILL_IMAGE)).sum())
    assert n_fills * (dl.dim // SUB_W) * (dl.dim // SUB_H) * 64 > 32 << 20
    want = pool.refs[idx]
    ctx = Context(0)  # its own density history: nothing measured at this scale yet
    results = []
    try:
        out = ctx.host_alloc((n, dl.dim, dl.dim, 4)) if pinned else np.empty((n, dl.dim, dl.dim, 4), dtype=np.uint8)
        try:
            for call in range(2):  # the first call measures, the second sizes its arenas from what the first measured
                out[:] = 0x5A
                results.append(ctx.render_batch_host(dl, out=out).copy())
        finally:
            if pinned:
                ctx.host_free(out)
    finally:
        ctx.close()
    # compared on copies, after the pinned buffer is gone: a failure report prints its arguments, and must not read freed memory
    for call, got in enumerate(results):
        _same(got, want, f"host-buffer call {call}, scale {scale}, {'pinned' if pinned else 'pageable'}")


# ---- the limit of the fill arena ---------------------------------------------------------------------------------------------


def test_scene_of_2_pow_28_fill_groups_is_refused(gpu_ctx, pools):
    """64 tiles x 2048 fills at scale 4, each from (-5, -5) to (W + 5, W + 5): 131 072 ops of 2048 groups, 2^28 groups in all
    (OSMT_MAX_FILL_GROUPS).  A list entry's 32-bit word index cannot reach the last of them, so the upload is refused with
    UNSUPPORTED and the count, by the sizing pass alone: nothing is allocated for the arenas and nothing is rendered.  The
    context renders a small batch afterwards.  The case just under the limit (2^28 - 2048 groups) would allocate about
    24 GiB of arenas and is deliberately not tested."""
    from osm_renderer_amd.lib import OsmtError

    scale, n_tiles, per_tile = 4, 64, 2048
    W = 256 * scale
    n_ops = n_tiles * per_tile
    jobs = np.zeros(n_tiles, JOB_DTYPE)
    jobs["x"], jobs["zoom"], jobs["has_canvas"] = np.arange(n_tiles), 15, 1
    jobs["n_ops"], jobs["op_off"] = per_tile, np.arange(n_tiles) * per_tile
    jobs["n_pts"], jobs["pt_off"] = 5, np.arange(n_tiles) * 5
    ops = np.zeros(n_ops, OP_DTYPE)  # the ops of a tile share its one ring
    ops["kind"], ops["opacity"], ops["n_rings"], ops["ring_off"] = abi.OP_FILL_COLOR, 0.5, 1, np.arange(n_ops) // per_tile
    ops["color"] = (np.arange(n_ops)[:, None] * np.array([1, 3, 7])) % 256
    rings = np.zeros(n_tiles, RING_DTYPE)
    rings["first_pt"], rings["n_pts"] = np.arange(n_tiles) * 5, 5
    coords = np.tile(np.array(_box(-5, -5, W + 5, W + 5), dtype=np.int32), (n_tiles, 1))
    dl = DisplayList(jobs, ops, rings, coords, np.zeros(0), abi.COORD_POINT_I32, scale)
    groups = n_ops * (W // SUB_W) * (W // SUB_H)
    assert groups == 2**28 == abi.MAX_FILL_GROUPS
    with pytest.raises(OsmtError) as e:
        gpu_ctx.upload(dl)
    assert e.value.code == abi.UNSUPPORTED and str(groups) in str(e.value) and "split the batch" in str(e.value), str(e.value)
    pool = pools(scale)
    scene = gpu_ctx.upload(pool.batch([Pool.EDGE, Pool.EMPTY]))
    got = gpu_ctx.render(scene).cpu().numpy()
    scene.free()
    _same(got, pool.refs[[Pool.EDGE, Pool.EMPTY]], "after the refusal")
