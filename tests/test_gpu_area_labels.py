"""Area labels of tile-built scenes on the GPU (osmt_scene_build_tile_labels_all, osm_renderer_amd/csrc/osmt_arealabels.hip):
registered area label bindings in, the labels of the ways and multipolygons of every tile of a scene of osmt_scene_build_tiles
out, in front of its node labels.

The batch the device built (osmt_scene_read_tile_area_labels) is compared BYTE FOR BYTE with the host mirror
osmt::area_labels_of_tile (host/osmt_arealabels.hpp through tests/arealabels_shim.cpp), which is written over GeodataReader's
own column walk, the stable sort_styled per kind and the literal merge loop, and is held against a Python restatement in
tests/test_area_labels_cpu.py.  The mirror takes its points from osmt_project and its anchors from osmt_label_positions_tiles
on the same device — the same functions as the kernels', so no rounding tie can separate them; an anchor the device declines
comes from the anchors' own host mirror.  way_sincos is compared with the mirror's and with labels.way_sincos of this
process.  The pixel cases compare a scene with device-built labels with the same scene given the mirror's batch through
osmt_scene_set_string_labels, and with the oracle's render of the host expansion of that batch."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from osm_renderer_amd import abi, labels, lib, styled
from osm_renderer_amd.display_list import DisplayList
from osm_renderer_amd.lib import OsmtError
from tests import _anchors as an
from tests import _arealabels as al
from tests import _text_placer_model as placer
from tests import _tilelabels as tl
from tests._styled_feed import geodata_of
from tests._tilequery import center_z18

pytestmark = pytest.mark.gpu

A = abi
MP = al.MP
CANVAS = (241, 238, 232)
CX, CY = center_z18()
NS = len(labels.SYNTH_GLYPHS)
ICONS = [(16, 16), (12, 20), (5, 7)]  # (height, width): 5 is odd
TEXTS = ["ABC", "", "HELLO KAFE", "A" * 40, "BD"]  # "A" * 40 is wider than every way here
GIDS = [0, 1 << 32, (1 << 64) - 1, 77, 78]


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.fixture(scope="module")
def tables(gpu_ctx):
    syn = labels.synth_glyph_table()
    gpu_ctx.register_glyphs(syn)
    shapes = [NS - 1] + [(g - 1) % (NS - 1) for g in range(1, 13)] + [NS - 1]
    cmap = [(0x20, 13)] + [(0x41 + i, 1 + i) for i in range(12)]
    font = labels.FontTable(cmap, [300] + [labels.SYNTH_GLYPHS[s][0] for s in shapes[1:]], [syn.first_id + s for s in shapes], [(1, 2, 17), (3, 5, -45)])
    gpu_ctx.register_font(font)
    rng = np.random.default_rng(23)
    imgs, ids = [], []
    for h, w in ICONS:
        img = rng.integers(0, 256, size=(h, w, 4)).astype(np.uint8)
        img[: h // 2, :, 3] = 255
        imgs.append(img)
        ids.append(gpu_ctx.register_image(img))
    return syn, font, imgs, ids


def _style_rows(font, ids):
    f = font.font_id
    return [
        dict(font_size=11.0, font_id=f),                                                       # 0: the kind's default position
        dict(layer=0, z_index=-0.0, icon=ids[2]),                                              # 1: ties with 0; icon only, of odd height
        dict(icon=ids[0], font_size=9.0, font_id=f, text_color=(150, 20, 60)),                 # 2: ties with 0 and 1; icon + default text
        dict(layer=-1, font_size=9.0, font_id=f, text_position=A.LABEL_POSITION_LINE),         # 3: explicit Line
        dict(z_index=2.5, font_size=13.0, font_id=f, text_color=(0, 90, 200), text_position=A.LABEL_POSITION_CENTER),  # 4: explicit Center
        dict(layer=1, text_style=True),                                                        # 5: no font size
        dict(layer=1, z_index=-3.0),                                                           # 6: neither icon nor text
        dict(layer=2, icon=ids[2], font_size=10.0, font_id=f, text_position=A.LABEL_POSITION_CENTER),  # 7: odd icon + Center text
    ]


class World:
    """an al.World with topology, tile index, Mercator factors and label styles registered, and draw styles bound to nothing"""

    def __init__(self, ctx, tables, path, w, draw=None):
        _, font, imgs, ids = tables
        self.ctx, self.w = ctx, w
        self.r, self.refs = w.write(path)
        self.g = geodata_of(self.r)
        self.gid = ctx.register_geodata(self.g)
        ctx.register_tile_index(self.gid, styled.TileIndex([(k, self.refs[k][1], self.refs[k][2]) for k in sorted(self.refs)]))
        self.ll = self.r.node_table()
        self.f = an.mercator_factors(self.ll)
        ctx.register_node_mercator(self.gid, self.f)
        st = np.zeros(1, styled.STYLE_REC_DTYPE)
        st["has_fill_color"], st["fill_color"], st["is_foreground_fill"] = 1, (170, 200, 150), 1
        first_draw = ctx.register_styles(st)
        draw = draw if draw is not None else [[] for _ in w.ways]
        self.draw_bind = ctx.register_style_bindings(styled.StyleBindings(self.gid, 0, 18, [[first_draw] * len(d) for d in draw], [[] for _ in w.mps]))
        rows = _style_rows(font, ids)
        self.add_styles(rows, [ICONS[ids.index(r["icon"])][0] if r.get("icon") is not None else 0 for r in rows], reset=True)
        self.mirrors = []

    def add_styles(self, rows, icon_h, reset=False):
        rec = tl.label_styles(rows)
        first = self.ctx.register_label_styles(rec)
        if reset:
            self.first = first
            self.styles, self.icon_h = np.zeros(first, styled.LABEL_STYLE_REC_DTYPE), [0] * first
        if first > len(self.styles):  # ids are the context's: another world registered styles in between
            pad = first - len(self.styles)
            self.styles, self.icon_h = np.concatenate([self.styles, np.zeros(pad, styled.LABEL_STYLE_REC_DTYPE)]), self.icon_h + [0] * pad
        assert first == len(self.styles)
        self.styles, self.icon_h = np.concatenate([self.styles, rec]), self.icon_h + list(icon_h)
        return first

    def bind(self, way_rows, mp_rows, zoom_lo=0, zoom_hi=18, texts=TEXTS, base=None):
        """registers an area label bindings table (style ids relative to `base`, default this world's first); returns (id, mirror)"""
        base = self.first if base is None else base
        fill = lambda rows, n: [[(s + base, t) for s, t in v] for v in rows] + [[] for _ in range(n - len(rows))]
        wb, mb = fill(way_rows, self.r.n_ways), fill(mp_rows, self.r.n_multipolygons)
        bid = self.ctx.register_area_label_bindings(styled.AreaLabelBindings(self.gid, zoom_lo, zoom_hi, wb, mb, texts))
        m = al.Mirror(self.r, wb, mb, texts, self.gid, zoom_lo, zoom_hi)
        self.mirrors.append(m)
        return bid, m

    def scene(self, tiles, scale=1):
        return self.ctx.build_tiles(styled.TileBatch(self.gid, tiles, {z: self.draw_bind for z in range(19)}, scale=scale, canvas=CANVAS))

    def anchors(self, tile, scale):
        """the anchor of every way and every multipolygon under `tile`, from the device; what it declines, from the host mirror"""
        n_w, n_m = self.r.n_ways, self.r.n_multipolygons
        reqs = [(i, 0) for i in range(n_w)] + [(i | MP, 0) for i in range(n_m)]
        pos = self.ctx.label_positions_tiles(self.gid, [tile], reqs, scale)
        for k in np.nonzero(pos["status"] == A.LABEL_TOO_LARGE)[0]:
            p = an.mirror_position(self.g, self.f, reqs[k][0], *tile, scale)
            pos[k] = (p["x"], p["y"], p["status"], 0)
        return pos[:n_w].copy(), pos[n_w:].copy()

    def want(self, tiles, mirror_of_zoom, scale=1):
        """the mirror's batch, its points taken from osmt_project and its anchors from osmt_label_positions_tiles on the device"""
        parts, memo = [], {}
        for z, x, y in tiles:
            if (z, x, y) not in memo:  # a tile may be listed many times
                pts = self.ctx.project(self.ll, z, x, y, float(scale)) if len(self.ll) else np.zeros((0, 2), np.int32)
                wp, mp = self.anchors((z, x, y), scale)
                memo[(z, x, y)] = mirror_of_zoom[z].labels(self.styles, self.icon_h, z, x, y, scale, pts, wp, mp)
            parts.append(memo[(z, x, y)])
        return al.batch_of(parts)

    def close(self):
        for m in self.mirrors:
            m.close()
        self.r.close()


def _same(got, want):
    assert got.job_label_off.tolist() == want.job_label_off.tolist()
    for name in ("labels", "runs", "chars", "way_pts", "way_sincos"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.shape == w.shape, name
        if not np.array_equal(_u8(g), _u8(w)):
            item = g.dtype.itemsize * (2 if name.startswith("way") else 1)
            bad = np.nonzero((_u8(g).reshape(-1, item) != _u8(w).reshape(-1, item)).any(1))[0]
            raise AssertionError(f"{name}: {len(bad)} of {len(g)} records differ, first at {int(bad[0])}: {g[bad[0]]} != {w[bad[0]]}")
    # the angles once more, with the libm of this process
    for r in got.runs[(got.labels["has_text"] == 1) & (got.runs["position"] == A.TEXT_LINE)]:
        a, n = int(r["pt_off"]), int(r["n_pts"])
        assert np.array_equal(_u8(got.way_sincos[a : a + n]), _u8(labels.way_sincos(got.way_pts[a : a + n])))


def _err(fn, code, *words):
    with pytest.raises(OsmtError) as e:
        fn()
    assert e.value.code == code and all(x in str(e.value) for x in words), str(e.value)


COUNTS = [1, 63, 64, 65, 2048, 2049]
SPOT0 = (CX + 100, CY)  # the count spots: a z18 tile each, 20 apart


@pytest.fixture(scope="module")
def shapes(gpu_ctx, tables, tmp_path_factory):
    """One world for the shape cases: the feature shapes around (CX, CY) and, per label count, a z18 tile of its own with one
    way and one multipolygon that share the count between them."""
    rng = np.random.default_rng(31)
    w = al.feature_world((CX, CY), GIDS)
    n_fw, n_fm = len(w.ways), len(w.mps)
    sq = lambda x, y, s: [(x, y), (x + s, y), (x + s, y + s), (x, y + s), (x, y)]
    way_rows = [[(int(s), None if rng.random() < 0.2 else int(rng.integers(0, len(TEXTS)))) for s in rng.choice(8, (0, 1, 3, 2)[i % 4], replace=False)]
                for i in range(n_fw)]
    way_rows[0] = [(2, 0), (7, 2), (1, None)]   # the closed way: two styles ask for its anchor (one request), one is icon only
    way_rows[1] = [(0, 0), (3, 3), (4, 4)]      # walked from its end: default Line, a text wider than the way, explicit Center
    way_rows[2] = [(0, 2)]                      # one node: Line places nothing, the record stays
    way_rows[3] = [(2, 0), (4, 0), (6, None)]   # no nodes: anchor NONE — no icon, y_offset 0, no centred text; Line with 0 points
    way_rows[4] = [(0, 0), (1, 0), (0, 4)]      # vertical; shares its global id and its rank with multipolygon 0: that one goes first
    way_rows[7] = [(3, 0), (5, 0)]              # a zero-length edge; a text style without a font size
    mp_rows = [[(0, 0), (2, 2), (3, 0)],        # default Center, icon + text, explicit Line on a multipolygon (nothing)
               [(0, 0)],                        # no polygons: never a candidate
               [(2, 0), (7, 1), (0, None)],     # first polygon empty: NONE
               [(4, 1), (1, None), (6, None)],  # an empty text, icon only, nothing
               [(7, 4)]]
    spots = {}
    for i, k in enumerate(COUNTS):
        t = (SPOT0[0] + 20 * i, SPOT0[1])
        wi = w.way(w.shape([(30, 40), (120, 70), (220, 60)], t), int(rng.integers(1, 1 << 63)), [t])
        way_rows.append([(int(rng.integers(0, 8)), None if j % 4 == 0 else int(j % len(TEXTS))) for j in range((k + 1) // 2)])
        mi = w.mp([w.polygon(w.shape(sq(60, 120, 50 + i), t))], int(rng.integers(1, 1 << 63)), [t])
        mp_rows.append([(int(rng.integers(0, 8)), None if j % 5 == 0 else int(j % len(TEXTS))) for j in range(k // 2)])
        spots[k] = t
        assert wi == len(way_rows) - 1 and mi == len(mp_rows) - 1
    W = World(gpu_ctx, tables, tmp_path_factory.mktemp("al") / "shapes.bin", w)
    W.spots, W.way_rows, W.mp_rows = spots, way_rows, mp_rows
    W.hi = W.bind(way_rows, mp_rows, 16, 18)
    W.lo = W.bind([list(reversed(b)) for b in way_rows], [list(reversed(b)) for b in mp_rows], 0, 15)  # other push order under the lower zooms
    yield W
    W.close()


def _tiles_of(W):
    t = [(18, *W.spots[k]) for k in COUNTS]
    t.insert(2, (18, CX + 7, CY + 300))  # no index tile near: no areas, in the middle
    t += [(18, CX, CY), (18, CX + 1, CY), (18, CX + 2, CY), (18, CX + 40, CY + 3)]  # entities of two tiles: an anchor per tile
    t += [(15, CX >> 3, CY >> 3), (12, CX >> 6, CY >> 6), (0, 0, 0)]  # mixed zooms, other bindings
    t += [(18, CX + 7, CY + 301)]  # no areas, at the end
    return t


@pytest.mark.parametrize("scale", [1, 2, 3, 4])
def test_built_batch_equals_the_mirror(gpu_ctx, shapes, scale):
    W = shapes
    tiles = _tiles_of(W)
    mir = {z: (W.hi[1] if z >= 16 else W.lo[1]) for z in range(19)}
    ids = {z: (W.hi[0] if z >= 16 else W.lo[0]) for z in range(19)}
    sc = W.scene(tiles, scale)
    got, node = sc.build_tile_labels_all(ids, None)
    want = W.want(tiles, mir, scale)
    _same(got, want)
    assert len(node.labels) == 0 and node.job_label_off.tolist() == [0] * (len(tiles) + 1)
    n = np.diff(want.job_label_off).tolist()
    assert n[:2] + n[3:7] == COUNTS and n[2] == 0 and n[-1] == 0  # the counts the case is about
    assert n[-2] == sum(len(b) for b in W.way_rows) + sum(len(b) for i, b in enumerate(W.mp_rows) if i != 1)  # zoom 0: the whole world
    lab, runs = want.labels, want.runs
    t0 = int(want.job_label_off[7])  # tile (18, CX, CY)
    near = lab[t0 : int(want.job_label_off[8])]
    nruns = runs[t0 : int(want.job_label_off[8])]
    assert ((near["has_icon"] == 0) & (near["has_text"] == 0)).any() and (nruns["y_offset"] == 2).any()  # 5 // 2
    assert ((nruns["position"] == A.TEXT_LINE) & (nruns["n_pts"] == 0)).any() and ((nruns["position"] == A.TEXT_LINE) & (nruns["n_pts"] == 1)).any()
    assert ((near["has_text"] == 1) & (near["n_segs"] == 0)).any() and ((near["has_text"] == 1) & (near["n_segs"] == 40)).any()
    line = nruns[nruns["position"] == A.TEXT_LINE]
    for r in line:  # walking order: never from the larger x
        if r["n_pts"] >= 2:
            p = want.way_pts[int(r["pt_off"]) : int(r["pt_off"]) + int(r["n_pts"])]
            assert p[0][0] <= p[-1][0]
    assert 1.0 in np.abs(want.way_sincos[:, 0]).tolist() and len(want.way_sincos) > 20  # a vertical edge: sin(-+pi/2)
    if scale == 2:
        assert set(np.unique(runs["font_size"]).tolist()) >= {0.0, 22.0, 26.0}
    assert len(sc.label_status()) == len(lab)
    sc.free()
    # 0 tiles
    sc = W.scene([], scale)
    got, node = sc.build_tile_labels_all(ids, None)
    assert len(got.labels) == 0 and got.job_label_off.tolist() == [0] and node.job_label_off.tolist() == [0]
    sc.free()


def test_order_and_anchor_rules_of_the_near_tile(gpu_ctx, shapes):
    """what the byte comparison above rests on, read out of the built batch itself"""
    W = shapes
    tile = (18, CX, CY)
    sc = W.scene([tile])
    got, _ = sc.build_tile_labels_all({18: W.hi[0]}, None)
    req = gpu_ctx.label_positions_stats()[0]
    wp, mp = W.anchors(tile, 1)
    # requests: once per (tile, entity) however many styles ask — ways 0, 3 (no nodes: asked, answered NONE), 4, and whichever of the
    # random rows ask; multipolygons 0, 2, 3 (1 has no polygons).  Counted from the rows:
    rows = [(False, i, b) for i, b in enumerate(W.way_rows[:8]) if i != 6] + [(True, i, b) for i, b in enumerate(W.mp_rows[:4]) if i != 1]

    def asks(mp_, s, t):
        st = W.styles[W.first + s]
        line = (not mp_) if st["text_position"] == A.LABEL_POSITION_NONE else st["text_position"] == A.LABEL_POSITION_LINE
        return bool(st["has_icon"]) or (bool(st["has_text_style"]) and bool(st["has_font_size"]) and t is not None and not line)

    assert req == sum(1 for mp_, i, b in rows if any(asks(mp_, s, t) for s, t in b)) and req >= 6
    assert wp[3]["status"] == A.LABEL_NONE and mp[2]["status"] == A.LABEL_NONE and mp[0]["status"] == A.LABEL_OK
    # multipolygon 0 and way 4 share global id 77; style 0 (None, +0.0) and style 1 (Some(0), -0.0) share a rank: the
    # multipolygon's default-Center text at ITS anchor comes in front of the way's labels, those in push order (0, 1, 0)
    lab, runs = got.labels, got.runs
    k = [i for i in range(len(lab)) if lab[i]["has_text"] and runs[i]["position"] == A.TEXT_CENTER and runs[i]["center_x"] == mp[0]["x"]
         and runs[i]["center_y"] == mp[0]["y"] and runs[i]["font_size"] == 11.0]
    assert len(k) == 1
    after = [(int(lab[i]["has_icon"]), int(lab[i]["has_text"]), int(lab[i]["n_segs"])) for i in range(k[0] + 1, k[0] + 5)]
    # the multipolygon's second style of that rank, then the way: "ABC" along it, the odd icon, "BD" along it
    assert after == [(1, 1, 10), (0, 1, 3), (1, 0, 0), (0, 1, 2)], after
    assert runs[k[0] + 3]["y_offset"] == 2 and runs[k[0] + 3]["center_x"] == wp[4]["x"]
    sc.free()


def test_too_large_is_refused_read_and_rebuilt_with_the_callers_anchor(gpu_ctx, tables, tmp_path_factory):
    w = al.World((CX, CY))
    rect = lambda x, y, a, b: [(x, y), (x + a, y), (x + a, y + b), (x, y + b), (x, y)]
    near, east = (CX, CY), (CX + 1, CY)
    w.way(w.shape(rect(20, 20, 60, 60)), 5, [near])
    strip = w.way(w.shape(rect(0.0, 0.0, 5000.0, 0.01)), 6, [near, east])  # 500 000 cells in the first grid
    w.mp([w.polygon(w.shape(rect(100, 100, 30, 30)))], 7, [near])
    W = World(gpu_ctx, tables, tmp_path_factory.mktemp("al") / "strip.bin", w)
    bid, m = W.bind([[(2, 0)], [(2, 0), (7, 4), (1, None)], []], [[(0, 0)]])
    tiles = [(18, CX + 9, CY + 9), (18, *near), (18, *east)]
    sc = W.scene(tiles)
    old = tl.string_labels([dict(chars="AB", font=tables[1].font_id, font_size=10.0, center=(50.0, 50.0))])
    old.job_label_off = np.array([0, 1, 1, 1], np.uint32)
    sc.set_string_labels(old)
    before = gpu_ctx.render(sc).cpu().numpy()
    _err(lambda: sc.build_tile_labels_all({18: bid}, None), A.UNSUPPORTED, "declined 2", "tile 1", f"way {strip}", "osmt_scene_read_declined_anchors")
    assert gpu_ctx.label_positions_stats()[2] == 2
    assert np.array_equal(gpu_ctx.render(sc).cpu().numpy(), before)  # the scene keeps the labels it had
    dec = sc.read_declined_anchors()
    assert [(int(d["tile"]), int(d["entity"]), int(d["status"])) for d in dec] == [(1, strip, A.LABEL_TOO_LARGE), (2, strip, A.LABEL_TOO_LARGE)]
    for d in dec:
        p = an.mirror_position(W.g, W.f, int(d["entity"]), *tiles[int(d["tile"])], 1)
        assert p["status"] == A.LABEL_OK
        d["x"], d["y"], d["status"] = p["x"], p["y"], p["status"]
    # half the overrides: the other pair is declined again, alone
    _err(lambda: sc.build_tile_labels_all({18: bid}, None, dec[:1]), A.UNSUPPORTED, "declined 1", "tile 2", f"way {strip}")
    assert len(sc.read_declined_anchors()) == 1
    got, _ = sc.build_tile_labels_all({18: bid}, None, dec)
    assert len(sc.read_declined_anchors()) == 0 and gpu_ctx.label_positions_stats()[2] == 0
    _same(got, W.want(tiles, {18: m}))
    mine = got.labels[int(got.job_label_off[1]) : int(got.job_label_off[2])]
    assert ((mine["has_icon"] == 1) & (mine["icon_center_x"] == dec[0]["x"]) & (mine["icon_center_y"] == dec[0]["y"])).sum() == 3
    assert not np.array_equal(gpu_ctx.render(sc).cpu().numpy(), before)
    # what an override list may not be
    bad = dec[::-1].copy()
    _err(lambda: sc.build_tile_labels_all({18: bid}, None, bad), A.INVALID_ARG, "anchor 1", "strictly ascending")
    bad = np.concatenate([dec[:1], dec[:1]])
    _err(lambda: sc.build_tile_labels_all({18: bid}, None, bad), A.INVALID_ARG, "strictly ascending")
    for v in (float("nan"), float("inf"), 2.0 ** 28 + 1):
        bad = dec.copy()
        bad[1]["y"] = v
        _err(lambda: sc.build_tile_labels_all({18: bid}, None, bad), A.INVALID_ARG, "anchor 1", "2^28")
    bad = dec.copy()
    bad[0]["status"] = A.LABEL_TOO_LARGE
    _err(lambda: sc.build_tile_labels_all({18: bid}, None, bad), A.INVALID_ARG, "anchor 0", "status 2")
    bad = dec.copy()
    bad[1]["tile"] = 3
    _err(lambda: sc.build_tile_labels_all({18: bid}, None, bad), A.INVALID_ARG, "anchor 1", "not a tile")
    bad = dec.copy()
    bad[1]["entity"] = 3
    _err(lambda: sc.build_tile_labels_all({18: bid}, None, bad), A.INVALID_ARG, "anchor 1", "way 3 out of range")
    # an override of status NONE, and one for a pair nobody asks about (ignored)
    none = dec.copy()
    none[0]["status"], none[0]["x"], none[0]["y"] = A.LABEL_NONE, 0.0, 0.0
    extra = np.concatenate([np.array([(0, 0, 1.0, 2.0, A.LABEL_OK, 0)], labels.AREA_ANCHOR_DTYPE), none])
    got, _ = sc.build_tile_labels_all({18: bid}, None, extra)
    mine = got.labels[int(got.job_label_off[1]) : int(got.job_label_off[2])]
    far = got.labels[int(got.job_label_off[2]) : int(got.job_label_off[3])]
    assert mine["has_icon"].sum() == 1 and far["has_icon"].sum() == 4  # tile 1: only the square's icon is left
    sc.free()
    W.close()


def test_cpp_binding_builds_reads_and_retries(gpu_ctx, tmp_path):
    """host/osmt_draw.hpp: TileScene::build_all_labels / read_tile_area_labels with osmt::HostAnchors in a program of their own
    (tests/arealabels_host_demo.cpp), which compares the batch it reads with osmt::area_labels_of_tile; the strip is declined by
    the device in two tiles and computed on the host"""
    w = al.feature_world((CX, CY), GIDS)
    rect = lambda x, y, a, b: [(x, y), (x + a, y), (x + a, y + b), (x, y + b), (x, y)]
    for _ in range(2):  # ids 8 and 9: the program binds way 9 to one style, (9 + 0) % 3 = 0, the icon
        strip = w.way(w.shape(rect(0.0, 0.0, 5000.0, 0.01)), 60 + len(w.ways), [(CX, CY), (CX + 1, CY)])
    assert strip == 9
    path = str(tmp_path / "w.bin")
    al.write_geodata(path, w.nodes, w.ways, w.polygons, w.mps, tile_refs=w.refs)
    tiles = [(18, CX, CY), (18, CX + 7, CY + 300), (18, CX + 1, CY), (15, CX >> 3, CY >> 3), (18, CX + 40, CY + 3)]
    for scale in (1, 2):
        out = subprocess.run([al.build_demo(), path, str(scale)] + [str(v) for t in tiles for v in t], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (out.stdout, out.stderr[-2000:])
        word, n_labels, on_host = out.stdout.split()
        assert word == "OK" and int(n_labels) > 40 and int(on_host) >= 3


def test_later_styles_and_bindings_and_every_combination_of_kinds(gpu_ctx, shapes, tables):
    W = shapes
    tiles = [(18, CX, CY), (18, *W.spots[65]), (18, CX + 1, CY)]
    _, font, _, ids = tables
    first = W.add_styles([dict(layer=-7, font_size=8.0, font_id=font.font_id), dict(layer=0, z_index=-1.0, icon=ids[0]), dict(layer=0, z_index=1.0)], [0, 16, 0])
    rng = np.random.default_rng(5)
    pick = lambda b: [(int(s) - 8 + first - W.first if s >= 8 else int(s), 0) for s in rng.choice(11, min(2, len(b) + 1), replace=False)]
    new = W.bind([pick(b) for b in W.way_rows], [pick(b) for b in W.mp_rows], 18, 18)
    sc = W.scene(tiles)
    _same(sc.build_tile_labels_all({18: new[0]}, None)[0], W.want(tiles, {18: new[1]}))
    _same(sc.build_tile_labels_all({18: W.hi[0]}, None)[0], W.want(tiles, {18: W.hi[1]}))  # an older table under the new ranks
    # nodes: a node index over this world's nodes and a binding for the first ten
    node_refs = {k: ([i for i in range(10)] if k == (CX, CY) else [], v[1], v[2]) for k, v in W.refs.items()}
    gpu_ctx.register_node_index(W.gid, tl.node_index_of(W.r, node_refs))
    nb = [[(W.first + 2, 0)], [(W.first + 4, 2), (W.first + 1, None)]] * 5 + [[]] * (W.r.n_nodes - 10)
    nid = gpu_ctx.register_label_bindings(styled.LabelBindings(W.gid, 0, 18, nb, TEXTS))
    area_only = W.want(tiles, {18: W.hi[1]})
    area, node = sc.build_tile_labels_all({18: W.hi[0]}, {18: nid})
    _same(area, area_only)
    alone = sc.build_tile_labels({18: nid})  # the node batch of the existing call
    for name in ("labels", "runs", "chars"):
        assert np.array_equal(_u8(getattr(node, name)), _u8(getattr(alone, name)))
    assert len(node.labels) == 15 * 2 and node.job_label_off.tolist() == alone.job_label_off.tolist()
    # both, attached: the same pixels and statuses as the host splice of the two batches
    sc.build_tile_labels_all({18: W.hi[0]}, {18: nid})
    out, st = gpu_ctx.render(sc).cpu().numpy(), sc.label_status()
    both = labels.splice_string_labels(area_only, alone)
    assert len(st) == len(both.labels)
    sc.set_string_labels(both)
    assert np.array_equal(gpu_ctx.render(sc).cpu().numpy(), out) and np.array_equal(sc.label_status(), st)
    # nodes only: the existing call's result; neither: no labels
    area, node = sc.build_tile_labels_all(None, {18: nid})
    assert len(area.labels) == 0 and len(node.labels) == 30 and len(sc.label_status()) == 30
    area, node = sc.build_tile_labels_all(None, None)
    assert len(area.labels) == 0 and len(node.labels) == 0 and len(sc.label_status()) == 0
    sc.free()


def test_refusals_name_their_offender(gpu_ctx, shapes, tables):
    W, L, h = shapes, lib.load(), gpu_ctx._h
    sc = W.scene([(18, *W.spots[1]), (10, 0, 0)])
    _err(lambda: sc.build_tile_labels_all({18: W.hi[0]}, None), A.INVALID_ARG, "tile 1", "zoom 10", "no area label bindings")
    _err(lambda: sc.build_tile_labels_all({18: W.hi[0], 10: W.hi[0]}, None), A.INVALID_ARG, "covers zooms 16..18")
    _err(lambda: sc.build_tile_labels_all({18: W.hi[0], 10: 1 << 20}, None), A.INVALID_ARG, "not registered")
    _err(lambda: sc.build_tile_labels_all({18: W.hi[0], 10: W.lo[0]}, {18: 1 << 20, 10: 1 << 20}), A.INVALID_ARG)  # the node half refuses: nothing is attached
    assert len(sc.label_status()) == 0
    up = gpu_ctx.upload(__import__("osm_renderer_amd.synth", fromlist=["x"]).config2(1))
    _err(lambda: up.build_tile_labels_all({z: W.hi[0] for z in range(19)}, None), A.INVALID_ARG, "not built by osmt_scene_build_tiles")
    up.free()
    sc.free()
    n_w, n_m = W.r.n_ways, W.r.n_multipolygons

    def bindings(way_rows, mp_rows=(), texts=TEXTS, gid=W.gid, n_ways=n_w, n_mps=n_m):
        fill = lambda rows, n: list(rows) + [[] for _ in range(n - len(rows))]
        b = styled.AreaLabelBindings(gid, 0, 18, fill(way_rows, n_ways), fill(mp_rows, n_mps), texts)
        d = b.as_desc()
        return lambda: lib.check(L.osmt_validate_area_label_bindings(C.byref(d), h)) or b

    bindings([[(W.first, 0), (W.first + 1, None)]], [[(W.first, 1)]])()
    _err(bindings([[(1 << 30, 0)]]), A.INVALID_ARG, "way_bindings[0].style", "not a registered label style")
    _err(bindings([], [[(1 << 30, 0)]]), A.INVALID_ARG, "multipolygon_bindings[0].style")
    _err(bindings([[(W.first, len(TEXTS))]]), A.INVALID_ARG, "text pool")
    _err(bindings([[(W.first, 0)]], texts=[[0xD800]]), A.INVALID_ARG, "U+D800")
    _err(bindings([[(W.first, 0)]], gid=1 << 20), A.INVALID_ARG, "is not registered")
    _err(bindings([[(W.first, 0)]] * (n_w + 1)), A.INVALID_ARG, "way_off")
    _err(bindings([], [[(W.first, 0)]] * (n_m + 1)), A.INVALID_ARG, "multipolygon_off")
    fresh = gpu_ctx.register_geodata(W.g)
    _err(bindings([[(W.first, 0)]], gid=fresh), A.INVALID_ARG, "no tile index")
    gpu_ctx.register_tile_index(fresh, styled.TileIndex([(k, W.refs[k][1], W.refs[k][2]) for k in sorted(W.refs)]))
    _err(bindings([[(W.first, 0)]], gid=fresh), A.INVALID_ARG, "no Mercator factors")
    gpu_ctx.register_node_mercator(fresh, W.f)
    other = gpu_ctx.register_area_label_bindings(bindings([[(W.first, 0)]], gid=fresh)())
    sc = W.scene([(18, CX, CY)])
    _err(lambda: sc.build_tile_labels_all({18: other}, None), A.INVALID_ARG, f"belongs to geodata id {fresh}, not {W.gid}")
    # the inspection calls
    _err(lambda: sc.read_tile_area_labels(), A.INVALID_ARG, "no device-built area labels")
    sc.build_tile_labels_all({18: W.hi[0]}, None)
    n, caps = (C.c_size_t * 3)(), (C.c_size_t * 3)(0, 0, 0)
    buf = np.zeros(1 << 16, np.uint8)
    assert L.osmt_scene_read_tile_area_labels(h, sc._h, C.c_void_p(buf.ctypes.data), None, None, None, None, None, caps, n) == A.INVALID_ARG
    assert L.osmt_scene_read_tile_area_labels(h, sc._h, C.c_void_p(buf.ctypes.data), None, None, None, None, None, None, n) == A.INVALID_ARG
    assert n[0] > 10 and n[2] > 4
    sc.free()


def test_limits_are_refused_with_the_exact_figure(gpu_ctx, shapes):
    W = shapes
    tile = (18, *W.spots[1])
    way = W.r.n_ways - len(COUNTS)  # the way of spot 1
    plain = 6  # neither icon nor text

    def table(k):
        rows = [[] for _ in range(way + 1)]
        rows[way] = [(plain, None)] * k
        return W.bind(rows, [], 18, 18)

    over, full = table(A.TILE_LABELS_MAX + 1), table(A.TILE_LABELS_MAX)
    sc = W.scene([(18, CX + 7, CY + 300), tile])
    _err(lambda: sc.build_tile_labels_all({18: over[0]}, None), A.UNSUPPORTED, "tile 1", "65537 area labels", "OSMT_TILE_LABELS_MAX")
    got, _ = sc.build_tile_labels_all({18: full[0]}, None)  # the limit itself builds, in the sort's device-memory tier
    assert np.diff(got.job_label_off).tolist() == [0, A.TILE_LABELS_MAX]
    _same(got, W.want([(18, CX + 7, CY + 300), tile], {18: full[1]}))
    _same(sc.build_tile_labels_all({18: W.hi[0]}, None)[0], W.want([(18, CX + 7, CY + 300), tile], {18: W.hi[1]}))  # and a correct build behind it
    sc.free()


# ---- pixels ---------------------------------------------------------------------------------------------------------
Z = 16
TX, TY = CX >> 2, CY >> 2


@pytest.fixture(scope="module")
def town(gpu_ctx, tables, tmp_path_factory):
    """10 x 7 tiles of zoom 16, each with a street (text along the way), a filled building with an icon and a centred name, a
    second building whose name collides with the first's, and a park multipolygon"""
    rng = np.random.default_rng(41)
    w = al.World((0, 0))
    way_rows, mp_rows, draw = [], [], []

    def shape(i, j, pts):  # fractions of the z16 tile (TX + i, TY + j)
        ids = []
        for fx, fy in pts:
            lat, lon = tl.latlon_of(Z, TX + i + fx, TY + j + fy)
            w.nodes.append((7000 + len(w.nodes), lat, lon, {}))
            ids.append(len(w.nodes) - 1)
        return ids

    box = lambda x, y, a, b: [(x, y), (x + a, y), (x + a, y + b), (x, y + b), (x, y)]
    for j in range(7):
        for i in range(10):
            k18 = [((TX + i) * 4 + 1, (TY + j) * 4 + 1)]
            gid = lambda: int(rng.integers(1, 1 << 60))
            street = [(0.9, 0.15 + 0.01 * (i % 3)), (0.6, 0.2), (0.35, 0.17), (0.08, 0.22)] if (i + j) % 2 else [(0.08, 0.2), (0.4, 0.16), (0.9, 0.21)]
            w.way(shape(i, j, street), gid(), k18)
            way_rows.append([(0, 2 if i % 4 else 3)])  # "HELLO KAFE" along the street; every fourth: a text wider than its way
            draw.append([])
            w.way(shape(i, j, box(0.2, 0.4, 0.25, 0.2)), gid(), k18)
            way_rows.append([(2, 0), (4, 4)])  # an icon with "ABC" below it along the outline... and "BD" at the anchor
            draw.append([0])
            w.way(shape(i, j, box(0.25, 0.45, 0.2, 0.15)), gid(), k18)
            way_rows.append([(7, 0)])  # its anchor lies in the first building's: the odd icon and "ABC" collide with it
            draw.append([])
            w.mp([w.polygon(shape(i, j, box(0.55, 0.55, 0.1, 0.1))), w.polygon(shape(i, j, box(0.6, 0.5, 0.3, 0.4)))], gid(), k18)
            mp_rows.append([(0, 2), (1, None)])  # the park's name at its centre, an icon
    W = World(gpu_ctx, tables, tmp_path_factory.mktemp("al") / "town.bin", w, draw)
    W.all = W.bind(way_rows, mp_rows)
    yield W
    W.close()


def _oracle_labels(sl, tables):
    syn, font = tables[0], tables[1]
    return placer.place_text_labels(sl.to_text_label_list(font)).to_label_list(syn)


def _latlon(dl):
    """a built scene's display list with per-point coordinates (DisplayList.subset re-packs those, not node references)"""
    return DisplayList(dl.jobs, dl.ops, dl.rings, dl.nodes[dl.coords], dl.dashes, abi.COORD_LATLON_F64, dl.scale)


def _images(tables):
    return [np.zeros((1, 1, 4), np.uint8)] * tables[3][0] + list(tables[2])


@pytest.mark.parametrize("scale", [1, 2])
@pytest.mark.parametrize("n_tiles", [5, 70])
def test_pixels_equal_the_mirror_fed_scene_and_the_oracle(gpu_ctx, oracle, tables, town, n_tiles, scale):
    W = town
    tiles = [(Z, TX + k % 10, TY + k // 10) for k in range(n_tiles)]
    sc = W.scene(tiles, scale)
    got, _ = sc.build_tile_labels_all({Z: W.all[0]}, None)
    want = W.want(tiles, {Z: W.all[1]}, scale)
    _same(got, want)
    assert len(want.labels) >= 6 * n_tiles  # a tile sees its neighbours' areas too
    lab, runs = want.labels, want.runs
    assert ((lab["has_text"] == 1) & (runs["position"] == A.TEXT_LINE) & (runs["n_pts"] >= 3)).sum() >= n_tiles and (lab["has_icon"] == 1).sum() >= 3 * n_tiles
    out = gpu_ctx.render(sc).cpu().numpy()
    st = sc.label_status()
    sc.set_string_labels(want)
    assert np.array_equal(gpu_ctx.render(sc).cpu().numpy(), out) and np.array_equal(sc.label_status(), st)
    sub = list(range(n_tiles)) if n_tiles <= 5 else list(range(0, n_tiles, 9))
    ll = _oracle_labels(want.subset(sub), tables)  # the host expansion of the compared tiles only: it is Python
    ref, rst = oracle.render_batch(_latlon(sc.dl).subset(sub), images=_images(tables), threads=min(8, len(sub)), labels=ll, want_status=True)
    lab_sub = np.concatenate([np.arange(int(want.job_label_off[i]), int(want.job_label_off[i + 1])) for i in sub])
    assert np.array_equal(st[lab_sub], rst)
    assert 0 in rst.tolist() and 1 in rst.tolist()  # a label fails and a label succeeds: the comparison is not vacuous
    assert np.array_equal(out[sub], ref)
    bare = W.scene([tiles[0]], scale)
    assert not np.array_equal(gpu_ctx.render(bare).cpu().numpy()[0], out[0])  # the labels are in the pixels
    bare.free()
    sc.free()
