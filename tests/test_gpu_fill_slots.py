"""k_prebin's fill role takes one PASS per wave: four consecutive slot descriptors (one per fill op and sub-tile row of
its window, written by k_opinfo — osmt_fill_slots.h), whichever ops they belong to.  Which wave builds a row changes no
pixel: every scene here is rendered through Context and its RGBA8 framebuffer compared bit for bit with the oracle —
passes that start and end in the middle of ops, passes of four ops, padding slots, fills far apart in the op list,
polygons that are not "simple" (several rings, more than 16 edges) sharing a pass with simple ones, rows with many
crossings, windows that must be halved, ops without a window, tiles without fills or without ops, slot reservations of
more than one k_opinfo workgroup, scales 2 and 4, and guessed arenas that turn out too small."""
import numpy as np
import pytest

from osm_renderer_amd import abi, display_list, synth
from osm_renderer_amd.display_list import TileBuilder

pytestmark = pytest.mark.gpu

SUB_H = 16


def _col(rnd):
    return tuple(int(v) for v in rnd.integers(0, 256, size=3))


def rows_polygon(x0, x1, sr0, n_sr, lean=7):
    """A quadrilateral whose records lie on exactly the sub-tile rows [sr0, sr0 + n_sr): rows ytop + 1 .. ybot carry records."""
    ytop, ybot = sr0 * SUB_H - 1, (sr0 + n_sr) * SUB_H - 1
    return [(x0, ytop), (x1, ytop + 2), (x1 - lean, ybot), (x0 + lean, ybot - 3), (x0, ytop)]


def star(cx, cy, r_out, r_in, n_tips, phase=0.0):
    a = phase + np.arange(2 * n_tips) * np.pi / n_tips
    r = np.where(np.arange(2 * n_tips) % 2 == 0, r_out, r_in)
    ring = np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], 1).round().astype(int).tolist()
    return ring + [ring[0]]


def mixed_heights_tile():
    """polygons of 1, 2, 3, 4, 5 and 16 sub-tile rows in one list: 31 slots, passes start and end in the middle of ops"""
    rnd = np.random.default_rng(71)
    tb = TileBuilder(x=1, canvas=(250, 246, 236))
    for i, n in enumerate([1, 2, 3, 4, 5, 16]):
        tb.fill(rows_polygon(10 + 35 * i, 60 + 35 * i, 0 if n == 16 else i % 3, n), _col(rnd), float(rnd.choice([1.0, 0.6, 0.35])))
    return tb.build()


def four_in_a_pass_tile():
    rnd = np.random.default_rng(72)
    tb = TileBuilder(x=2, canvas=(236, 246, 250))
    for i in range(4):
        tb.fill(rows_polygon(20 + 50 * i, 90 + 50 * i, 3 + 2 * i, 1), _col(rnd), 0.7)
    return tb.build()


def one_polygon_tile():
    """one slot and three empty padding slots"""
    tb = TileBuilder(x=3, canvas=(240, 240, 240))
    tb.fill(rows_polygon(100, 180, 7, 1), (200, 30, 60), 0.8)
    return tb.build()


def fills_between_strokes_tile():
    """fills separated by 40 stroke ops each"""
    rnd = np.random.default_rng(73)
    tb = TileBuilder(x=4, canvas=(244, 240, 228))
    for i in range(3):
        tb.fill(rows_polygon(30 + 60 * i, 120 + 60 * i, 2 + 3 * i, 2 + i), _col(rnd), 0.6)
        for k in range(40):
            p = rnd.integers(0, 256, size=2)
            tb.stroke([p.tolist(), (p + rnd.integers(-30, 31, size=2) + [1, 0]).tolist()], float(rnd.choice([1.0, 3.0])), _col(rnd), 0.8)
    tb.fill(rows_polygon(5, 250, 14, 2), _col(rnd), 0.5)
    return tb.build()


def not_simple_tile():
    """a two-ring polygon and a 17-edge polygon share passes with simple ones (slots 1 + 3 + 1 + 3 + 1 + 5)"""
    rnd = np.random.default_rng(74)
    tb = TileBuilder(x=5, canvas=(230, 236, 242))
    tb.fill(rows_polygon(10, 70, 1, 1), _col(rnd), 0.7)
    tb.fill([rows_polygon(60, 200, 2, 3), [(90, 40), (170, 44), (160, 70), (95, 66), (90, 40)]], _col(rnd), 0.8)  # with a hole
    tb.fill(rows_polygon(150, 250, 4, 1), _col(rnd), 0.6)
    ring17 = star(128, 150, 15, 9, 8, 0.2)[:-1]
    ring17 = ring17 + [(ring17[0][0] + 3, ring17[0][1] + 2), ring17[0]]
    assert len(ring17) - 1 == 17
    tb.fill(ring17, _col(rnd), 0.9)
    tb.fill(rows_polygon(20, 120, 12, 1), _col(rnd), 0.5)
    tb.fill(star(60, 200, 38, 12, 9), _col(rnd), 0.75)  # 18 edges
    return tb.build()


def crossings_tile():
    """a simple star (16 edges) whose middle rows cross eight times, a 40-tip star over the whole tile whose 64 rows of a pass hold
    far more than 384 crossings (the window is halved), and a simple polygon next to them"""
    rnd = np.random.default_rng(75)
    tb = TileBuilder(x=6, canvas=(252, 250, 240))
    ring = []
    for k in range(8):  # a comb: eight teeth, 16 edges
        ring += [(20 + 12 * k, 38), (26 + 12 * k, 70)]
    ring = ring[:16] + [ring[0]]
    assert len(ring) - 1 == 16
    tb.fill(ring, _col(rnd), 0.8)
    tb.fill(star(128, 128, 140, 20, 40, 0.05), _col(rnd), 0.5)
    tb.fill(rows_polygon(180, 240, 10, 2), _col(rnd), 0.7)
    return tb.build()


def outside_tile():
    """a polygon wholly outside the tile between two that are inside; one whose rows are inside but whose columns are not"""
    tb = TileBuilder(x=7, canvas=(10, 20, 30))
    tb.fill(rows_polygon(30, 90, 2, 2), (250, 200, 10), 0.9)
    tb.fill([(300, 300), (380, 310), (340, 390), (300, 300)], (1, 2, 3), 1.0)
    tb.fill([(-90, 40), (-20, 44), (-50, 120), (-90, 40)], (9, 9, 9), 1.0)
    tb.fill([(20, -80), (90, -70), (50, -1), (20, -80)], (7, 7, 7), 1.0)  # y1 = -1: no row inside
    tb.fill(rows_polygon(100, 200, 9, 3), (20, 200, 250), 0.6)
    return tb.build()


def strokes_only_tile():
    rnd = np.random.default_rng(76)
    tb = TileBuilder(x=8, canvas=(200, 220, 210))
    for _ in range(9):
        p = rnd.integers(20, 236, size=2)
        tb.stroke([p.tolist(), (p + [25, -14]).tolist(), (p + [40, 9]).tolist()], 3.0, _col(rnd), 0.8, cap=abi.CAP_ROUND)
    return tb.build()


def empty_tile():
    return TileBuilder(x=9, canvas=(1, 2, 3)).build()


def six_hundred_polygons_tile():
    """600 small polygons: ops 511 and 512 belong to two k_opinfo workgroups, whose reservations each end on a pass boundary"""
    rnd = np.random.default_rng(77)
    tb = TileBuilder(x=10, canvas=(238, 238, 230))
    for i in range(600):
        cx, cy = (int(v) for v in rnd.integers(0, 256, size=2))
        r = int(rnd.integers(3, 14))
        tb.fill([(cx - r, cy - r), (cx + r, cy - r // 2), (cx + r // 2, cy + r), (cx - r, cy + r // 3), (cx - r, cy - r)], _col(rnd),
                float(rnd.choice([1.0, 0.6, 0.3])))
    return tb.build()


def scale_tile(scale):
    """polygons up to the whole height of the tile (16 * scale slots per op), a two-ring one and small ones"""
    W = 256 * scale
    rnd = np.random.default_rng(780 + scale)
    tb = TileBuilder(x=11, scale=scale, canvas=(246, 240, 236))
    tb.fill([(-5, -5), (W + 5, -3), (W - 9, W + 5), (4, W + 2), (-5, -5)], _col(rnd), 0.3)
    tb.fill(rows_polygon(W // 5, W // 2, 3, 16 * scale - 5, lean=9 * scale), _col(rnd), 0.6)
    tb.fill([rows_polygon(W // 2, W - 10, 1, 8 * scale, lean=3), star(3 * W // 4, 4 * SUB_H * scale, 20 * scale, 8 * scale, 5)], _col(rnd), 0.7)
    for i in range(9):
        tb.fill(rows_polygon(10 + 25 * i * scale, 40 + 25 * i * scale, 16 * scale - 1 - (i % 3), 1), _col(rnd), 0.8)
    tb.fill(star(W // 3, 2 * W // 3, 60 * scale, 15 * scale, 30), _col(rnd), 0.5)
    return tb.build()


SINGLE = {"heights": mixed_heights_tile, "four": four_in_a_pass_tile, "one": one_polygon_tile, "between": fills_between_strokes_tile,
          "not_simple": not_simple_tile, "crossings": crossings_tile, "outside": outside_tile, "strokes": strokes_only_tile,
          "empty": empty_tile, "six_hundred": six_hundred_polygons_tile}


class Tiles:
    """Every scale-1 tile of this file with its oracle framebuffer, rendered once."""

    def __init__(self, oracle):
        self.names = list(SINGLE)
        self.dls = [SINGLE[n]() for n in self.names]
        self.refs = oracle.render_batch(display_list.concat(self.dls), images=(), threads=8)
        self.config2 = synth.make_tiles(synth.config_tiles(60), zoom=15, coord_kind=abi.COORD_POINT_I32)
        self.config2_ref = oracle.render_batch(self.config2, images=(), threads=8)

    def get(self, name):
        i = self.names.index(name)
        return self.dls[i], self.refs[i]


@pytest.fixture(scope="module")
def tiles(oracle):
    return Tiles(oracle)


def _check(gpu_ctx, dl, want, msg):
    scene = gpu_ctx.upload(dl)
    got = gpu_ctx.render(scene).cpu().numpy()
    scene.free()
    want = np.asarray(want).reshape(got.shape)
    bad = np.nonzero((got != want).any(axis=-1))
    assert len(bad[0]) == 0, (f"{msg}: {len(bad[0])} pixels differ; first (tile,y,x)={tuple(int(b[0]) for b in bad)} "
                              f"gpu={got[bad][0].tolist()} oracle={want[bad][0].tolist()}")


def _fill_slots(dl):
    """slots of a scale-1 tile: sub-tile rows of every fill's bounding rows clipped to the tile (None for a fill without a window)"""
    out = []
    for op in dl.ops:
        if op["kind"] != abi.OP_FILL_COLOR:
            continue
        ys, xs = [], []
        for r in range(int(op["ring_off"]), int(op["ring_off"]) + int(op["n_rings"])):
            p0, n = int(dl.rings[r]["first_pt"]), int(dl.rings[r]["n_pts"])
            pts = np.asarray(dl.coords).reshape(-1, 2)[p0:p0 + n]
            xs += pts[:, 0].tolist()
            ys += pts[:, 1].tolist()
        ylo, yhi = max(min(ys) + 1, 0), min(max(ys), 255)
        xlo, xhi = max(min(xs), 0), min(max(xs), 255)
        out.append((yhi // SUB_H) - (ylo // SUB_H) + 1 if ylo <= yhi and xlo <= xhi else None)
    return out


def test_the_tiles_are_what_they_claim(tiles):
    """the shapes above land on the slots their docstrings name (host arithmetic only)"""
    assert _fill_slots(tiles.get("heights")[0]) == [1, 2, 3, 4, 5, 16]
    assert _fill_slots(tiles.get("four")[0]) == [1, 1, 1, 1]
    assert _fill_slots(tiles.get("one")[0]) == [1]
    assert _fill_slots(tiles.get("between")[0]) == [2, 3, 4, 2]
    assert _fill_slots(tiles.get("not_simple")[0]) == [1, 3, 1, 3, 1, 5]
    assert _fill_slots(tiles.get("crossings")[0]) == [3, 16, 2]
    assert _fill_slots(tiles.get("outside")[0]) == [2, None, None, None, 3]
    assert _fill_slots(tiles.get("strokes")[0]) == [] and len(tiles.get("strokes")[0].ops) == 9
    assert len(tiles.get("empty")[0].ops) == 0
    six = tiles.get("six_hundred")[0]
    assert len(six.ops) == 600 and all(s for s in _fill_slots(six)[500:520])


@pytest.mark.parametrize("name", [n for n in SINGLE if n != "six_hundred"])
def test_single_tiles(gpu_ctx, tiles, name):
    dl, ref = tiles.get(name)
    _check(gpu_ctx, dl, ref[None], name)


def test_six_hundred_polygons_across_two_workgroups(gpu_ctx, tiles):
    dl, ref = tiles.get("six_hundred")
    _check(gpu_ctx, dl, ref[None], "600 polygons")


def test_batch_of_70_tiles_with_lists(gpu_ctx, tiles):
    """more than 64 tiles: lists from k_sublist; the scene is sized exactly, so the fill blocks are made from the pass count"""
    dl = display_list.concat(tiles.dls + [tiles.config2])
    assert dl.n_jobs == 70
    _check(gpu_ctx, dl, np.concatenate([tiles.refs, tiles.config2_ref]), "70 tiles")


def test_batch_of_8_tiles_folded(gpu_ctx, tiles):
    """at most 64 tiles: small tiles get their lists from k_raster's own waves; worst-case arenas, fill blocks stride through the passes"""
    names = ["heights", "four", "one", "between", "not_simple", "crossings", "outside"]
    parts = [tiles.get(n) for n in names]
    dl = display_list.concat([p[0] for p in parts] + [tiles.config2.subset([0])])
    assert dl.n_jobs == 8
    _check(gpu_ctx, dl, np.concatenate([np.stack([p[1] for p in parts]), tiles.config2_ref[:1]]), "8 tiles")


@pytest.mark.parametrize("scale", [2, 4])
def test_scales_2_and_4(gpu_ctx, oracle, scale):
    dl = scale_tile(scale)
    ref = oracle.render_batch(dl, images=(), threads=1)
    _check(gpu_ctx, dl, ref, f"scale {scale}")


def test_guessed_arenas_too_small_store_empty_slots_and_render_again(oracle):
    """Host-buffer calls guess their arenas from recent uploads.  A batch with ten times the geometry overflows the guess: the
    fill ops whose arena words are refused keep their slots and store them empty, the slot array (sized from the same guess)
    drops what lies past it, the error word says so and the call renders again with exact sizes — bit for bit the same as
    a scene that was sized exactly from the start."""
    from osm_renderer_amd.renderer import Context

    ctx = Context(0)  # its own density history
    try:
        small = synth.make_tiles(synth.config_tiles(96, x0=20100, y0=11100), radius=(1.0, 3.0), step=3.0)
        big = synth.make_tiles(synth.config_tiles(96, x0=20100, y0=11100))
        ctx.render_batch_host(small)  # measures: small densities
        ctx.render_batch_host(small)  # guessed, fits
        got_big = ctx.render_batch_host(big)  # guessed from the small batches: misses, rendered again
        scene = ctx.upload(big)  # public scenes are always sized exactly
        want_big = ctx.render(scene).cpu().numpy()
        scene.free()
        assert np.array_equal(got_big, want_big)
        pick = [3, 50, 94]
        assert np.array_equal(want_big[pick], oracle.render_batch(big.subset(pick), threads=3))
    finally:
        ctx.close()
