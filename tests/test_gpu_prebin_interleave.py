"""k_prebin's grid holds stroke blocks (OSMT_BIN_SEGS virtual segments each) spread evenly among fill groups
(osmt_prebin_roles.h).  Which block does what changes no pixel: every scene here is rendered through Context and its
RGBA8 framebuffer compared bit for bit with the oracle — scenes with only one of the two roles, totals of virtual
segments on both sides of a block boundary for 16, 32 and 64 segments per block, lopsided tiles, and a mix of them as a
large batch (lists from k_sublist) and as a small one (lists folded into k_raster).  Tiles are at scale 1."""
import numpy as np
import pytest

from osm_renderer_amd import abi, display_list, synth
from osm_renderer_amd.display_list import TileBuilder

pytestmark = pytest.mark.gpu

VSEG_TOTALS = [15, 16, 17, 31, 32, 33, 63, 64, 65, 129]
CAPS = [abi.CAP_NONE, abi.CAP_BUTT, abi.CAP_ROUND, abi.CAP_SQUARE]


def n_vsegs(dl):
    """Virtual segments of a display list: the edges of every stroke op plus two cap stubs where it has round or square caps."""
    total = 0
    for op in dl.ops:
        if op["kind"] != abi.OP_STROKE:
            continue
        for r in range(int(op["ring_off"]), int(op["ring_off"]) + int(op["n_rings"])):
            total += max(int(dl.rings[r]["n_pts"]) - 1, 0)
        if op["cap"] in (abi.CAP_ROUND, abi.CAP_SQUARE):
            total += 2
    return total


def _walk(rnd, n_edges, reach=22):
    """n_edges + 1 points inside the tile, no two consecutive ones equal"""
    p = rnd.integers(30, 226, size=2)
    pts = [p.tolist()]
    while len(pts) < n_edges + 1:
        q = np.clip(p + rnd.integers(-reach, reach + 1, size=2), -10, 266)
        if (q != p).any():
            pts.append(q.tolist())
            p = q
    return pts


def _col(rnd):
    return tuple(int(v) for v in rnd.integers(0, 256, size=3))


def _blob(rnd, r_max=40):
    c = rnd.integers(0, 256, size=2)
    n = int(rnd.integers(3, 9))
    a = np.sort(rnd.uniform(0, 2 * np.pi, size=n))
    r = rnd.uniform(3, r_max, size=n)
    ring = np.stack([c[0] + r * np.cos(a), c[1] + r * np.sin(a)], 1).round().astype(int).tolist()
    return ring + [ring[0]]


def strokes_only_tile():
    rnd = np.random.default_rng(41)
    tb = TileBuilder(x=1, canvas=(250, 246, 236))
    for i in range(23):
        tb.stroke(_walk(rnd, int(rnd.integers(1, 9))), float(rnd.choice([0.5, 1.0, 2.5, 6.0])), _col(rnd), float(rnd.choice([1.0, 0.6])),
                  dashes=[5.0, 3.0] if i % 4 == 0 else None, cap=CAPS[i % 4], use_caps_for_dashes=(i % 8 == 0))
    return tb.build()


def fills_only_tile():
    rnd = np.random.default_rng(42)
    tb = TileBuilder(x=2, canvas=(236, 246, 250))
    for _ in range(31):  # an odd count: the last fill group holds one op
        tb.fill(_blob(rnd), _col(rnd), float(rnd.choice([1.0, 0.7, 0.4])))
    return tb.build()


def vseg_total_tile(total):
    """Strokes whose virtual segments number exactly `total` (a round-capped one, 5 + 2; a square-capped one, 3 + 2; one
    polyline with the rest), a few fills between them."""
    rnd = np.random.default_rng(1000 + total)
    tb = TileBuilder(x=3, y=total, canvas=(244, 240, 228))
    tb.fill(_blob(rnd), _col(rnd), 0.8)
    tb.stroke(_walk(rnd, 5), 3.0, _col(rnd), 0.9, cap=abi.CAP_ROUND)
    tb.fill(_blob(rnd), _col(rnd), 0.5)
    tb.stroke(_walk(rnd, total - 12), 2.0, _col(rnd), 0.7, dashes=[7.0, 4.0] if total % 2 else None)
    tb.stroke(_walk(rnd, 3), 5.0, _col(rnd), 0.6, cap=abi.CAP_SQUARE)
    tb.fill(_blob(rnd), _col(rnd), 1.0)
    dl = tb.build()
    assert n_vsegs(dl) == total
    return dl


def many_segments_tile():
    """one polygon, 300 stroke edges (a 100-edge way among them) and their cap stubs"""
    rnd = np.random.default_rng(43)
    tb = TileBuilder(x=4, canvas=(240, 240, 240))
    tb.fill(_blob(rnd, 90), _col(rnd), 0.6)
    tb.stroke(_walk(rnd, 100, reach=12), 2.0, _col(rnd), 0.8, cap=abi.CAP_ROUND)
    for i in range(40):
        tb.stroke(_walk(rnd, 5), float(rnd.choice([1.0, 2.0, 4.0])), _col(rnd), float(rnd.choice([1.0, 0.5])), cap=CAPS[i % 4],
                  dashes=[4.0, 4.0] if i % 5 == 0 else None)
    dl = tb.build()
    assert 300 <= n_vsegs(dl) <= 345
    return dl


def many_polygons_tile():
    """300 polygons and one stroke segment, in the middle of them"""
    rnd = np.random.default_rng(44)
    tb = TileBuilder(x=5, canvas=(230, 236, 242))
    for i in range(300):
        if i == 150:
            tb.stroke([(20, 30), (230, 210)], 4.0, (200, 40, 40), 0.8)
        tb.fill(_blob(rnd, 25), _col(rnd), float(rnd.choice([1.0, 0.6, 0.3])))
    dl = tb.build()
    assert n_vsegs(dl) == 1
    return dl


def empty_tile():
    return TileBuilder(x=6, canvas=(1, 2, 3)).build()


def config2_tiles(n):
    return synth.make_tiles(synth.config_tiles(n), zoom=15, coord_kind=abi.COORD_POINT_I32)


class Tiles:
    """Every tile of this file with its oracle framebuffer, rendered once."""

    def __init__(self, oracle):
        self.dls, self.refs, self.names = [], [], {}
        named = [("strokes", strokes_only_tile()), ("fills", fills_only_tile()), ("segments", many_segments_tile()),
                 ("polygons", many_polygons_tile()), ("empty", empty_tile())]
        named += [(f"v{t}", vseg_total_tile(t)) for t in VSEG_TOTALS]
        for name, dl in named:
            self.names[name] = len(self.dls)
            self.dls.append(dl)
            self.refs.append(oracle.render_batch(dl, images=(), threads=1)[0])
        self.config2 = config2_tiles(49)
        self.config2_ref = oracle.render_batch(self.config2, images=(), threads=8)

    def get(self, name):
        i = self.names[name]
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


@pytest.mark.parametrize("name", ["strokes", "fills"])
def test_one_role_only(gpu_ctx, tiles, name):
    dl, ref = tiles.get(name)
    assert (n_vsegs(dl) == 0) == (name == "fills")
    assert all(op["kind"] == (abi.OP_STROKE if name == "strokes" else abi.OP_FILL_COLOR) for op in dl.ops)
    _check(gpu_ctx, dl, ref[None], name)


@pytest.mark.parametrize("total", VSEG_TOTALS)
def test_virtual_segment_totals_around_block_boundaries(gpu_ctx, tiles, total):
    dl, ref = tiles.get(f"v{total}")
    assert n_vsegs(dl) == total
    _check(gpu_ctx, dl, ref[None], f"{total} virtual segments")


@pytest.mark.parametrize("name", ["segments", "polygons"])
def test_lopsided_tiles(gpu_ctx, tiles, name):
    dl, ref = tiles.get(name)
    _check(gpu_ctx, dl, ref[None], name)


MIX = ["strokes", "fills", "v33", "v129", "segments", "polygons", "empty"]


def test_mixed_batch_of_70_tiles_with_lists(gpu_ctx, tiles):
    """more than 64 tiles: every tile's lists come from k_sublist"""
    names = MIX + [f"v{t}" for t in VSEG_TOTALS if t not in (33, 129)] + ["empty"] * 6
    parts = [tiles.get(n) for n in names]
    dl = display_list.concat([p[0] for p in parts] + [tiles.config2])
    assert dl.n_jobs == 70
    _check(gpu_ctx, dl, np.concatenate([np.stack([p[1] for p in parts]), tiles.config2_ref]), "70 tiles")


def test_mixed_batch_of_8_tiles_folded(gpu_ctx, tiles):
    """at most 64 tiles: tiles of at most 128 ops get their lists from k_raster's own waves"""
    parts = [tiles.get(n) for n in MIX]
    one = config2_tiles(1)
    dl = display_list.concat([p[0] for p in parts] + [one])
    assert dl.n_jobs == 8
    _check(gpu_ctx, dl, np.concatenate([np.stack([p[1] for p in parts]), tiles.config2_ref[:1]]), "8 tiles")
