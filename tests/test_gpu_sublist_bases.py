"""Where k_sublist puts a tile's lists in the entry arena (osmt_list_slices.h) changes no pixel.  Batches of 1, 8 and 64
tiles (small batches: only a tile of more than 128 ops gets lists at all), of 65 and 70 (every tile gets lists, one
cursor) and of 300 (sixteen cursors, each with a slice of the arena, and the overflow slice) are rendered and compared
with the oracle bit for bit.  The batches have empty tiles at the start, in the middle and at the end, and one tile
whose lists are far longer than a slice holds, so that it and the later tiles of its slice land in the overflow slice.
The library has no read-back of the list entries, so the pixels are what is compared: an entry out of place or out of
order shows there (`over` is not commutative and the tiles' colours differ)."""
import numpy as np
import pytest

from osm_renderer_amd import abi, display_list, synth
from osm_renderer_amd.display_list import TileBuilder

pytestmark = pytest.mark.gpu

N_POOL = 10
CAPS = [abi.CAP_NONE, abi.CAP_BUTT, abi.CAP_ROUND, abi.CAP_SQUARE]


def _col(rnd):
    return tuple(int(v) for v in rnd.integers(0, 256, size=3))


def _blob(rnd, r_max):
    c = rnd.integers(0, 256, size=2)
    n = int(rnd.integers(3, 8))
    a = np.sort(rnd.uniform(0, 2 * np.pi, size=n))
    r = rnd.uniform(3, r_max, size=n)
    ring = np.stack([c[0] + r * np.cos(a), c[1] + r * np.sin(a)], 1).round().astype(int).tolist()
    return ring + [ring[0]]


def _walk(rnd, n_edges):
    p = rnd.integers(20, 236, size=2)
    pts = [p.tolist()]
    while len(pts) < n_edges + 1:
        q = np.clip(p + rnd.integers(-30, 31, size=2), -10, 266)
        if (q != p).any():
            pts.append(q.tolist())
            p = q
    return pts


def small_tile(i):
    """two or three dozen ops that overlap: fills of all opacities, plain and dashed strokes"""
    rnd = np.random.default_rng(7000 + i)
    tb = TileBuilder(x=10 + i, canvas=_col(rnd))
    for k in range(int(rnd.integers(20, 37))):
        if k % 3 == 2:
            tb.stroke(_walk(rnd, int(rnd.integers(1, 5))), float(rnd.choice([1.0, 2.5, 5.0])), _col(rnd), float(rnd.choice([1.0, 0.6])),
                      dashes=[6.0, 3.0] if k % 9 == 2 else None, cap=CAPS[k % 4])
        else:
            tb.fill(_blob(rnd, 45), _col(rnd), float(rnd.choice([1.0, 0.7, 0.35])))
    return tb.build()


def long_tile():
    """150 polygons that each reach most of the tile's 128 sub-tiles, and strokes across them: ~19 000 list entries"""
    rnd = np.random.default_rng(7100)
    tb = TileBuilder(x=50, canvas=(200, 210, 220))
    for k in range(150):
        x0, y0 = (int(v) for v in rnd.integers(-5, 40, size=2))
        x1, y1 = (int(v) for v in rnd.integers(215, 262, size=2))
        tb.fill([(x0, y0), (x1, y0 + 3), (x1 - 4, y1), (x0 + 2, y1 - 5), (x0, y0)], _col(rnd), float(rnd.choice([1.0, 0.2, 0.05])))
        if k % 10 == 0:
            tb.stroke([(0, 5 + k), (256, 250 - k)], 3.0, _col(rnd), 0.7)
    return tb.build()


def empty_tile():
    return TileBuilder(x=60, canvas=(9, 8, 7)).build()


class Pool:
    """the distinct tiles of this file and their oracle framebuffers, rendered once"""

    def __init__(self, oracle):
        self.dls = [small_tile(i) for i in range(N_POOL)] + [long_tile(), empty_tile()]
        self.LONG, self.EMPTY = N_POOL, N_POOL + 1
        self.refs = oracle.render_batch(display_list.concat(self.dls), images=(), threads=8)

    def batch(self, idx):
        return display_list.concat([self.dls[i] for i in idx]), self.refs[list(idx)]


@pytest.fixture(scope="module")
def pool(oracle):
    return Pool(oracle)


def layout(pool, n, shift=0):
    """n tile indices into the pool: empty tiles first, in the middle and last, the long tile early (so that the tiles of
    its slice that come later find the slice's cursor past its end), the small tiles in turn everywhere else"""
    idx = [(k + shift) % N_POOL for k in range(n)]
    idx[0] = pool.EMPTY
    idx[-1] = pool.EMPTY
    if n >= 8:
        idx[1] = pool.EMPTY
        idx[n // 2] = pool.EMPTY
        idx[n // 2 + 1] = pool.EMPTY
        idx[5] = pool.LONG
    if n >= 64:
        idx[5 + 32] = pool.LONG  # with sixteen cursors: the same one again
        idx[n - 2] = pool.EMPTY
    return idx


def _render(gpu_ctx, dl, stream=None):
    scene = gpu_ctx.upload(dl)
    got = gpu_ctx.render(scene, stream=stream)
    return scene, got


def _same(got, want, msg):
    bad = np.nonzero((got != want).any(axis=-1))
    assert len(bad[0]) == 0, (f"{msg}: {len(bad[0])} pixels differ; first (tile,y,x)={tuple(int(b[0]) for b in bad)} "
                              f"gpu={got[bad][0].tolist()} oracle={want[bad][0].tolist()}")


@pytest.mark.parametrize("n", [1, 8, 64, 65, 70, 300])
def test_batch_sizes(gpu_ctx, pool, n):
    idx = layout(pool, n) if n > 1 else [pool.LONG]
    dl, want = pool.batch(idx)
    assert dl.n_jobs == n
    scene, got = _render(gpu_ctx, dl)
    got = got.cpu().numpy()
    scene.free()
    _same(got, want, f"{n} tiles")


def test_all_tiles_empty_but_one(gpu_ctx, pool):
    """299 tiles reserve nothing; the one that does is the last of its slice"""
    idx = [pool.EMPTY] * 300
    idx[293] = pool.LONG
    dl, want = pool.batch(idx)
    scene, got = _render(gpu_ctx, dl)
    got = got.cpu().numpy()
    scene.free()
    _same(got, want, "one long tile among empty ones")


def test_two_scenes_in_flight_on_two_streams(gpu_ctx, pool):
    import torch

    dl_a, want_a = pool.batch(layout(pool, 300))
    dl_b, want_b = pool.batch(layout(pool, 257, shift=3))
    s_a, s_b = torch.cuda.Stream(), torch.cuda.Stream()
    sc_a, sc_b = gpu_ctx.upload(dl_a), gpu_ctx.upload(dl_b)
    out_a = out_b = None
    for _ in range(3):  # the scenes' cursors and counts are cleared and used again by every render
        out_a = gpu_ctx.render(sc_a, out_a, stream=s_a)
        out_b = gpu_ctx.render(sc_b, out_b, stream=s_b)
    s_a.synchronize()
    s_b.synchronize()
    got_a, got_b = out_a.cpu().numpy(), out_b.cpu().numpy()
    sc_a.free()
    sc_b.free()
    _same(got_a, want_a, "stream a")
    _same(got_b, want_b, "stream b")


def test_arenas_guessed_too_small_are_reported_and_rendered_again(oracle):
    """The one way an arena can be too small: a host-buffer call sizes its arenas (the list arena among them) from the
    densities of earlier calls.  With 160 tiles the list arena is in slices; a batch with ten times the geometry of the
    ones before does not fit the guess, the kernels say so in the scene's error word — they write nothing outside their
    arenas — and the call renders again with exact sizes.  What this can and cannot show: k_opinfo refuses the ops whose
    fill groups or stroke records do not fit, so the list counts shrink with them and the error word usually carries the
    fill or stroke arena's bit, not the list arena's; any of them leads to the same second render.  That a sliced arena
    refuses a tile only when both its slice and the overflow slice are full, and places every other tile inside the
    arena, is what tests/test_list_slices_cpu.py checks on the functions the kernel calls."""
    from osm_renderer_amd.renderer import Context

    ctx = Context(0)  # its own density history
    try:
        small = synth.make_tiles(synth.config_tiles(160, x0=21000, y0=12000), radius=(1.0, 3.0), step=3.0)
        big = synth.make_tiles(synth.config_tiles(160, x0=21000, y0=12000))
        ctx.render_batch_host(small)  # measures
        got_small = ctx.render_batch_host(small)  # guessed, fits
        got_big = ctx.render_batch_host(big)  # guessed from the small batches: misses, rendered again
        pick = [0, 16, 85, 159]
        assert np.array_equal(got_big[pick], oracle.render_batch(big.subset(pick), threads=4))
        assert np.array_equal(got_small[pick], oracle.render_batch(small.subset(pick), threads=4))
        scene = ctx.upload(big)
        want_big = ctx.render(scene).cpu().numpy()
        scene.free()
        assert np.array_equal(got_big, want_big)
    finally:
        ctx.close()
