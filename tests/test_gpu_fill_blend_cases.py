"""The cases at which a shortcut in k_raster's fill blend (blend_masked: new = s + (1 - o) * old under the coverage mask)
would go wrong, compared with the oracle bit for bit — RGBA8, packed RGB8 and the f64 canvas — at scale 1 and 2, on a
canvas and without one (accumulators that start at +0.0), as a small batch (lists folded into k_raster) and as a batch
of 70 tiles (lists from k_sublist, the other instantiation of the kernel).

Two such shortcuts were built and measured (writing the colour of a fill of opacity exactly 1.0, branching
over row pairs no lane covers); they were exact and not faster, and are not in the kernel.  The cases stay: opacities
on both sides of the test such a shortcut makes (1.0, the double below it, 0.5, 0.0), colours 0 and 255, fills that
leave most row pairs of a sub-tile empty, image fills with alpha 1.0 and below, and one tile with more fills in a
sub-tile than a chunk stages (the blend then takes its coverage words from global memory)."""
import numpy as np
import pytest

from osm_renderer_amd import abi, display_list
from osm_renderer_amd.display_list import TileBuilder

pytestmark = pytest.mark.gpu

BELOW_ONE = float(np.nextafter(1.0, 0.0))
OPACITIES = [1.0, BELOW_ONE, 0.5, 0.0]


def _sc(pts, s):
    return [(int(x) * s, int(y) * s) for x, y in pts]


def _rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)]


def opacities_tile(s, canvas, x):
    """four overlapping columns of each opacity, in colours 0, 255 and in between, each crossed by bars of every opacity"""
    tb = TileBuilder(x=x, scale=s, canvas=canvas)
    cols = [(0, 0, 0), (255, 255, 255), (255, 0, 128), (17, 200, 99)]
    for i, o in enumerate(OPACITIES):
        tb.fill(_sc(_rect(8 + 60 * i, 5, 80 + 60 * i, 250), s), cols[i], o)
    for i, o in enumerate(OPACITIES):
        tb.fill(_sc(_rect(0, 20 + 55 * i, 256, 50 + 55 * i), s), cols[(i + 1) % 4], o)
    for i, o in enumerate(reversed(OPACITIES)):
        tb.fill(_sc([(30 + 50 * i, 10), (90 + 50 * i, 128), (30 + 50 * i, 245), (10 + 50 * i, 128), (30 + 50 * i, 10)], s), cols[(i + 2) % 4], o)
    return tb.build()


def order_tile(s, canvas, x, opaque_last):
    """an opaque fill over a translucent one over a stroke, or the three the other way round"""
    tb = TileBuilder(x=x, scale=s, canvas=canvas)
    steps = [
        lambda: tb.stroke(_sc([(10, 30), (120, 140), (245, 90)], s), 9.0 * s, (200, 30, 30), 0.8, cap=abi.CAP_ROUND),
        lambda: tb.fill(_sc([(20, 20), (230, 40), (200, 220), (40, 200), (20, 20)], s), (30, 90, 220), 0.45),
        lambda: tb.fill(_sc([(60, 10), (250, 120), (100, 250), (60, 10)], s), (0, 255, 0), 1.0),
    ]
    for st in (steps if opaque_last else steps[::-1]):
        st()
    tb.stroke(_sc([(0, 128), (256, 130)], s), 3.0 * s, (0, 0, 0), 1.0)  # a stroke over whatever came out
    return tb.build()


def partial_rows_tile(s, canvas, x):
    """opaque fills that leave row pairs of their sub-tiles empty: a sliver one pixel high, a triangle inside one row pair,
    a polygon over exactly one sub-tile, one over a sub-tile and parts of its neighbours; the same again translucent"""
    tb = TileBuilder(x=x, scale=s, canvas=canvas)
    for o, dy in ((1.0, 0), (0.6, 128)):
        tb.fill(_sc(_rect(3, 9 + dy, 250, 10 + dy), s), (255, 255, 0), o)
        tb.fill(_sc([(40, 34 + dy), (47, 34 + dy), (43, 36 + dy), (40, 34 + dy)], s), (0, 0, 255), o)
        tb.fill(_sc(_rect(64, 48 + dy, 96, 64 + dy), s), (255, 0, 0), o)
        tb.fill(_sc(_rect(120, 40 + dy, 170, 75 + dy), s), (0, 0, 0), o)
        tb.fill(_sc([(200, 30 + dy), (250, 31 + dy), (201, 33 + dy), (200, 30 + dy)], s), (255, 255, 255), o)
    return tb.build()


def image_tile(s, canvas, x, ids):
    """an icon whose alpha is 1.0 everywhere and one with every alpha, over and under colour fills"""
    tb = TileBuilder(x=x, scale=s, canvas=canvas)
    tb.fill(_sc(_rect(10, 10, 200, 200), s), (90, 10, 10), 1.0)
    tb.fill_image(_sc([(20, 20), (240, 60), (180, 240), (30, 180), (20, 20)], s), ids[0])
    tb.fill_image(_sc([(5, 100), (250, 110), (120, 250), (5, 100)], s), ids[1])
    tb.fill(_sc(_rect(100, 0, 140, 256), s), (255, 255, 255), 1.0)
    tb.fill_image(_sc(_rect(90, 90, 160, 93), s), ids[1])
    return tb.build()


def crowded_tile(s, canvas, x):
    """40 fills in the same sub-tiles: more than a chunk of 16 stages"""
    rnd = np.random.default_rng(77)
    tb = TileBuilder(x=x, scale=s, canvas=canvas)
    for i in range(40):
        cx, cy = (int(v) for v in rnd.integers(60, 120, size=2))
        w, h = (int(v) for v in rnd.integers(2, 40, size=2))
        col = [(0, 0, 0), (255, 255, 255)][i % 2] if i % 5 == 0 else tuple(int(v) for v in rnd.integers(0, 256, size=3))
        tb.fill(_sc([(cx - w, cy - h), (cx + w, cy - h // 2), (cx + w // 2, cy + h), (cx - w, cy - h)], s), col, OPACITIES[i % 3] if i % 7 else 0.0)
    return tb.build()


def make_icons(rnd):
    solid = rnd.integers(0, 256, size=(5, 7, 4), dtype=np.uint8)
    solid[..., 3] = 255
    mixed = rnd.integers(0, 256, size=(9, 4, 4), dtype=np.uint8)
    mixed[0, 0, 3], mixed[1, 1, 3], mixed[2, 2, 3] = 0, 255, 254
    return solid, mixed


class Scenes:
    def __init__(self, gpu_ctx):
        solid, mixed = make_icons(np.random.default_rng(5))
        ids = [gpu_ctx.register_image(solid), gpu_ctx.register_image(mixed)]
        self.images = [np.zeros((1, 1, 4), np.uint8)] * ids[0] + [solid] + [np.zeros((1, 1, 4), np.uint8)] * (ids[1] - ids[0] - 1) + [mixed]
        self.ids = ids
        self._cache = {}

    def tiles(self, s, canvas):
        key = (s, canvas)
        if key not in self._cache:
            self._cache[key] = [opacities_tile(s, canvas, 1), order_tile(s, canvas, 2, True), order_tile(s, canvas, 3, False),
                                partial_rows_tile(s, canvas, 4), image_tile(s, canvas, 5, self.ids), crowded_tile(s, canvas, 6)]
        return self._cache[key]


@pytest.fixture(scope="module")
def scenes(gpu_ctx):
    return Scenes(gpu_ctx)


def _bits_equal(a, b):
    return (np.ascontiguousarray(a).view(np.uint64) == np.ascontiguousarray(b).view(np.uint64))


def _check_all_outputs(gpu_ctx, oracle, dl, images, msg, f64_jobs):
    want = oracle.render_batch(dl, images=images, threads=min(8, dl.n_jobs))
    scene = gpu_ctx.upload(dl)
    got = gpu_ctx.render(scene).cpu().numpy()
    f64 = gpu_ctx.render_f64(scene).cpu().numpy()
    scene.free()
    bad = np.nonzero((got != want).any(axis=-1))
    assert len(bad[0]) == 0, (f"{msg} RGBA8: {len(bad[0])} pixels differ; first (tile,y,x)={tuple(int(b[0]) for b in bad)} "
                              f"gpu={got[bad][0].tolist()} oracle={want[bad][0].tolist()}")
    for j in f64_jobs:
        _, ref = oracle.render_job(dl, j, images=images, want_f64=True)
        same = _bits_equal(f64[j], ref)
        assert same.all(), f"{msg}: f64 canvas differs on tile {j} at {np.argwhere(~same)[0].tolist()}"
    rgb = gpu_ctx.render_batch_rgb(dl).reshape(dl.n_jobs, dl.dim, dl.dim, 3)
    bad = np.nonzero((rgb != want[..., :3]).any(axis=-1))
    assert len(bad[0]) == 0, f"{msg} RGB8: {len(bad[0])} pixels differ; first (tile,y,x)={tuple(int(b[0]) for b in bad)}"


@pytest.mark.parametrize("canvas", [(241, 238, 232), (0, 0, 0), None], ids=["canvas", "black_canvas", "no_canvas"])
@pytest.mark.parametrize("scale", [1, 2])
def test_fills_match_the_oracle_in_every_output(gpu_ctx, oracle, scenes, scale, canvas):
    tiles = scenes.tiles(scale, canvas)
    dl = display_list.concat(tiles)
    assert dl.n_jobs == 6 and all(int(j["n_ops"]) <= 128 for j in dl.jobs)  # a small batch: k_raster's waves build the lists
    _check_all_outputs(gpu_ctx, oracle, dl, scenes.images, f"scale {scale} canvas {canvas}", range(dl.n_jobs))


def test_fills_match_the_oracle_with_lists_from_k_sublist(gpu_ctx, oracle, scenes):
    """70 tiles (more than a small batch holds): the kernel without folded lists"""
    tiles = scenes.tiles(1, (241, 238, 232)) + scenes.tiles(1, None)
    dl = display_list.concat([tiles[i % len(tiles)] for i in range(70)])
    assert dl.n_jobs == 70
    _check_all_outputs(gpu_ctx, oracle, dl, scenes.images, "70 tiles", range(12))


def test_opacity_one_leaves_the_colour_itself(gpu_ctx, oracle):
    """the f64 canvas under an opaque fill is the fill's colour itself, c / 255, in every bit; one ulp less opacity
    leaves a trace of what was below"""
    tb = TileBuilder(canvas=(255, 255, 255))
    tb.fill(_rect(0, 0, 256, 256), (10, 20, 30), 0.3)
    tb.fill(_rect(0, 0, 128, 256), (77, 0, 255), 1.0)
    tb.fill(_rect(128, 0, 256, 256), (77, 0, 255), BELOW_ONE)
    dl = tb.build()
    scene = gpu_ctx.upload(dl)
    f64 = gpu_ctx.render_f64(scene).cpu().numpy()[0]
    scene.free()
    _, ref = oracle.render_job(dl, 0, want_f64=True)
    assert _bits_equal(f64, ref).all()
    col = np.array([77, 0, 255], dtype=np.float64) / 255.0
    inner = slice(8, 248)  # away from the polygons' edges
    assert _bits_equal(f64[inner, 8:120, :3], np.broadcast_to(col, (240, 112, 3))).all()
    assert not _bits_equal(f64[inner, 136:248, :3], np.broadcast_to(col, (240, 112, 3))).all(axis=-1).any()
