"""Node labels of tile-built scenes on the GPU (osmt_scene_build_tile_labels, osm_renderer_amd/csrc/osmt_tilelabels.hip): a
registered node index + registered label styles and label bindings in, the label pass of a scene of osmt_scene_build_tiles out.

The batch the device built (osmt_scene_read_tile_labels) is compared BYTE FOR BYTE with the host mirror
osmt::node_labels_of_tile (host/osmt_tilelabels.hpp through tests/tilelabels_shim.cpp), which is written over GeodataReader's
own column walk and the stable sort_styled and is held against a Python restatement in tests/test_tile_labels_cpu.py.  The
mirror takes its points from osmt_project on the same device — the same function as the kernel's, so no rounding tie can
separate them; the libm projection is held against the oracle's in the CPU file.  The pixel cases compare a scene with
device-built labels with the same scene given the mirror's batch through osmt_scene_set_string_labels, and with the oracle's
render of the host expansion of that batch, the way tests/test_gpu_text_labels.py compares."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from osm_renderer_amd import abi, labels, lib, styled
from osm_renderer_amd.display_list import DisplayList
from osm_renderer_amd.lib import OsmtError
from tests import _text_placer_model as placer
from tests import _tilelabels as tl
from tests._styled_feed import geodata_of
from tests._tilequery import center_z18

pytestmark = pytest.mark.gpu

A = abi
CANVAS = (241, 238, 232)
CX, CY = center_z18()
W = tl.WORLD
NS = len(labels.SYNTH_GLYPHS)
ICONS = [(16, 16), (12, 20), (5, 7)]  # (height, width): 5 is odd
TEXTS = ["ABC", "", "HELLO KAFE", "A" * 40, "BD"]


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
        dict(font_size=11.0, font_id=f),                                                       # 0
        dict(layer=0, z_index=-0.0, icon=ids[2]),                                              # 1: ties with 0; the icon of odd height
        dict(icon=ids[0], font_size=9.0, font_id=f, text_color=(150, 20, 60)),                 # 2: ties with 0 and 1
        dict(layer=-1, font_size=9.0, font_id=f, text_position=A.LABEL_POSITION_LINE),         # 3: Line on a node
        dict(z_index=2.5, font_size=13.0, font_id=f, text_color=(0, 90, 200), text_position=A.LABEL_POSITION_CENTER),
        dict(layer=1, text_style=True),                                                        # 5: no font size
        dict(layer=1, z_index=-3.0),                                                           # 6: neither icon nor text
        dict(layer=2, icon=ids[1], font_size=10.0, font_id=f),                                 # 7
    ]


class World:
    """a geodata file of nodes (and optional ways) with topology, tile index, node index, label styles and empty area bindings registered"""

    def __init__(self, ctx, tables, path, nodes, refs, ways=(), area_style=None, shuffle=None):
        _, font, imgs, ids = tables
        self.ctx, self.nodes = ctx, nodes
        self.r, self.refs = tl.make_world(path, nodes, refs, ways)
        self.gid = ctx.register_geodata(geodata_of(self.r))
        ctx.register_tile_index(self.gid, styled.TileIndex([(k, self.refs[k][1], []) for k in sorted(self.refs)]))
        ctx.register_node_index(self.gid, tl.node_index_of(self.r, self.refs, shuffle))
        st = np.zeros(1, styled.STYLE_REC_DTYPE)
        st["has_fill_color"], st["fill_color"], st["is_foreground_fill"] = 1, (170, 200, 150), 1
        first_area = ctx.register_styles(st)
        self.area_bind = ctx.register_style_bindings(styled.StyleBindings(self.gid, 0, 18, [[first_area]] * len(ways), []))
        self.add_styles(_style_rows(font, ids), [ICONS[ids.index(r["icon"])][0] if r.get("icon") is not None else 0 for r in _style_rows(font, ids)],
                        reset=True)
        self.ll = self.r.node_table()
        self.mirrors = []

    def add_styles(self, rows, icon_h, reset=False):
        rec = tl.label_styles(rows)
        first = self.ctx.register_label_styles(rec)
        if reset:
            self.first = first
            self.styles, self.icon_h = np.zeros(first, styled.LABEL_STYLE_REC_DTYPE), [0] * first
        assert first == len(self.styles)
        self.styles, self.icon_h = np.concatenate([self.styles, rec]), self.icon_h + list(icon_h)
        return first

    def bind(self, node_bindings, zoom_lo=0, zoom_hi=18, texts=TEXTS, base=None):
        """registers a label bindings table (style ids relative to `base`, default this world's first); returns (id, mirror)"""
        base = self.first if base is None else base
        nb = [[(s + base, t) for s, t in v] for v in node_bindings]
        nb += [[]] * (self.r.n_nodes - len(nb))
        bid = self.ctx.register_label_bindings(styled.LabelBindings(self.gid, zoom_lo, zoom_hi, nb, texts))
        m = tl.Mirror(self.r, nb, texts, self.gid, zoom_lo, zoom_hi)
        self.mirrors.append(m)
        return bid, m

    def scene(self, tiles, scale=1):
        return self.ctx.build_tiles(styled.TileBatch(self.gid, tiles, {z: self.area_bind for z in range(19)}, scale=scale, canvas=CANVAS))

    def want(self, tiles, mirror_of_zoom, scale=1):
        """the mirror's batch, its points taken from osmt_project on the device"""
        parts, memo = [], {}
        for z, x, y in tiles:
            if (z, x, y) not in memo:  # a tile may be listed many times
                pts = self.ctx.project(self.ll, z, x, y, float(scale))
                memo[(z, x, y)] = mirror_of_zoom[z].labels(self.styles, self.icon_h, z, x, y, scale, pts)
            parts.append(memo[(z, x, y)])
        return tl.batch_of(parts)

    def close(self):
        for m in self.mirrors:
            m.close()
        self.r.close()


def _same(got, want):
    assert got.job_label_off.tolist() == want.job_label_off.tolist()
    for name in ("labels", "runs", "chars"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.shape == w.shape, name
        if not np.array_equal(_u8(g), _u8(w)):
            item = g.dtype.itemsize
            bad = np.nonzero((_u8(g).reshape(-1, item) != _u8(w).reshape(-1, item)).any(1))[0]
            raise AssertionError(f"{name}: {len(bad)} of {len(g)} records differ, first at {int(bad[0])}: {g[bad[0]]} != {w[bad[0]]}")


def _spread(rng, k, i0, n_styles=8, n_texts=len(TEXTS)):
    """bindings of nodes i0 .. that sum to k labels: nodes with 3 bindings, a rest, and a node with none"""
    out = []
    while k > 0:
        n = min(3, k)
        out.append([(int(s), None if (len(out) + j) % 4 == 0 else int((i0 + len(out) + j) % n_texts)) for j, s in enumerate(rng.choice(n_styles, n, replace=False))])
        k -= n
    return out + [[]]


COUNTS = [1, 63, 64, 65, 2048, 2049]


@pytest.fixture(scope="module")
def shapes(gpu_ctx, tables, tmp_path_factory):
    """One world for the shape cases: per label count a z18 tile of its own (20 tiles apart), two tiles of 8192 and 8193 node
    references, one node listed by all nine tiles of a neighbourhood, nodes in the four corners of the world."""
    rng = np.random.default_rng(31)
    nodes, refs, bind = [], {}, []

    def node(tx, ty, gid=None):
        lat, lon = tl.latlon_of(18, tx + rng.random(), ty + rng.random())
        nodes.append((int(rng.integers(1, 1 << 63)) if gid is None else gid, lat, lon))
        return len(nodes) - 1

    spots = {}
    for i, k in enumerate(COUNTS):
        tx, ty = CX + 20 * i, CY
        b = _spread(rng, k, len(nodes))
        refs[(tx, ty)] = [node(tx, ty) for _ in b]
        bind += b
        spots[k] = (tx, ty)
    for j, n_refs in enumerate((8192, 8193)):  # candidates before dedup: the sort's LDS boundary
        tx, ty = CX + 20 * j, CY + 40
        ids = [node(tx, ty) for _ in range(40)]
        bind += _spread(rng, 3 * 39, len(nodes))[:40]
        refs[(tx, ty)] = [ids[k % 40] for k in range(n_refs)]
        spots[n_refs] = (tx, ty)
    nine = node(CX + 200, CY, gid=(1 << 64) - 1)
    bind.append([(4, 2), (7, 0), (2, 4)])
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            refs.setdefault((CX + 200 + dx, CY + dy), []).append(nine)
    for gid, (tx, ty) in zip((0, 1 << 32, 1 << 63, 77), ((0, 0), (W - 1, 0), (0, W - 1), (W - 1, W - 1))):
        refs[(tx, ty)] = [node(tx, ty, gid), node(tx, ty)]
        bind += [[(0, 0), (1, 1), (2, None)], [(2, 2)]]
    w = World(gpu_ctx, tables, tmp_path_factory.mktemp("tl") / "shapes.bin", nodes, refs, shuffle=rng)
    w.spots, w.nine, w.bind_rows = spots, nine, bind
    w.hi = w.bind(bind, 16, 18)
    low = [list(reversed(b)) for b in bind]  # other push order under the lower zooms
    w.lo = w.bind(low, 0, 15)
    yield w
    w.close()


def _tiles_of(w):
    t = [(18, *w.spots[k]) for k in COUNTS]
    t.insert(2, (18, CX + 7, CY + 300))  # no index tile near: 0 nodes, in the middle
    t += [(18, *w.spots[8192]), (18, *w.spots[8193]), (18, CX + 200, CY), (18, CX + 201, CY + 1)]
    t += [(18, 0, 0), (18, W - 1, 0), (18, 0, W - 1), (18, W - 1, W - 1), (10, 0, 0), (10, 1023, 1023)]
    t += [(15, (CX + 20) >> 3, CY >> 3), (12, CX >> 6, CY >> 6), (0, 0, 0)]  # mixed zooms, other bindings
    t += [(18, CX + 7, CY + 301)]  # 0 nodes, at the end
    return t


@pytest.mark.parametrize("scale", [1, 2, 3, 4])
def test_built_batch_equals_the_mirror(gpu_ctx, shapes, scale):
    w = shapes
    tiles = _tiles_of(w)
    mir = {z: (w.hi[1] if z >= 16 else w.lo[1]) for z in range(19)}
    ids = {z: (w.hi[0] if z >= 16 else w.lo[0]) for z in range(19)}
    sc = w.scene(tiles, scale)
    got = sc.build_tile_labels(ids)
    want = w.want(tiles, mir, scale)
    _same(got, want)
    n = np.diff(want.job_label_off).tolist()
    assert n[:2] + n[3:7] == COUNTS and n[2] == 0 and n[-1] == 0  # the counts the case is about
    assert n[9] == 3 and n[10] == 3  # the node of nine tiles, once, from its own tile and from a neighbour
    assert n[-2] == sum(len(b) for b in w.bind_rows)  # zoom 0: the whole world
    lab, runs = want.labels, want.runs
    assert (lab["has_text"] == 1).any() and ((lab["has_text"] == 1) & (lab["n_segs"] == 0)).any()  # empty text
    assert ((lab["has_icon"] == 0) & (lab["has_text"] == 0)).any() and (runs["y_offset"] == 2).any()  # 5 // 2
    assert len(want.chars) > 4 * 256  # the char scan crosses several blocks
    if scale == 2:
        assert set(np.unique(runs["font_size"]).tolist()) >= {0.0, 22.0, 26.0}
    assert len(sc.label_status()) == len(lab)
    sc.free()
    # 0 tiles
    sc = w.scene([], scale)
    got = sc.build_tile_labels(ids)
    assert len(got.labels) == 0 and got.job_label_off.tolist() == [0]
    sc.free()


def test_tiles_without_candidates_and_labels_without_chars(gpu_ctx, shapes):
    """the empty ends of the pipeline: tiles but no candidate at all (nothing to gather, sort or expand), and labels whose
    chars add up to zero (nothing to copy)"""
    w = shapes
    far = [(18, CX + 7, CY + 300), (18, CX + 9, CY + 400), (12, 5, 5)]
    ids = {z: (w.hi[0] if z >= 16 else w.lo[0]) for z in range(19)}
    sc = w.scene(far)
    got = sc.build_tile_labels(ids)
    assert len(got.labels) == 0 and len(got.chars) == 0 and got.job_label_off.tolist() == [0, 0, 0, 0]
    sc.free()
    tile = (18, *w.spots[65])
    rows = [[(1, 0), (6, 2), (5, 3)] for _ in w.bind_rows]  # an icon, nothing, a text style without a font size: no text anywhere
    plain = w.bind(rows, 18, 18)
    sc = w.scene([far[0], tile])
    got = sc.build_tile_labels({18: plain[0]})
    _same(got, w.want([far[0], tile], {18: plain[1]}))
    assert len(got.labels) == 3 * len(w.refs[tile[1:]][0]) and len(got.chars) == 0 and not got.labels["has_text"].any()
    gpu_ctx.render(sc)
    assert len(sc.label_status()) == len(got.labels)
    sc.free()


def test_cpp_binding_builds_and_reads_the_same_batch(shapes, tmp_path):
    """host/osmt_draw.hpp: Context::register_node_index / register_label_styles / register_label_bindings and
    TileScene::build_tile_labels / read_tile_labels in a program of their own (tests/tilelabels_host_demo.cpp), which compares
    the batch it reads with osmt::node_labels_of_tile"""
    w = shapes
    path = str(tmp_path / "w.bin")
    tl.write_geodata(path, [(g, la, lo, {}) for g, la, lo in w.nodes], [], [], [], tile_refs=w.refs)
    tiles = [(18, *w.spots[65]), (18, CX + 7, CY + 300), (18, *w.spots[2049]), (15, (CX + 20) >> 3, CY >> 3), (18, 0, 0)]
    for scale in (1, 2):
        out = subprocess.run([tl.build_demo(), path, str(scale)] + [str(v) for t in tiles for v in t], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (out.stdout, out.stderr[-2000:])
        word, n_labels, n_chars = out.stdout.split()
        assert word == "OK" and int(n_labels) > 1000 and int(n_chars) == 0


def test_later_styles_move_every_rank(gpu_ctx, shapes, tables):
    w = shapes
    tiles = [(18, *w.spots[65]), (18, *w.spots[2049]), (18, CX + 200, CY)]
    _, font, _, ids = tables
    first = w.add_styles([dict(layer=-7, font_size=8.0, font_id=font.font_id), dict(layer=0, z_index=-1.0, icon=ids[0]), dict(layer=0, z_index=1.0)], [0, 16, 0])
    rng = np.random.default_rng(5)
    rows = [[(int(s) - 8 + first - w.first if s >= 8 else int(s), 0) for s in rng.choice(11, 2, replace=False)] for _ in w.bind_rows]
    new = w.bind(rows, 18, 18)
    sc = w.scene(tiles)
    _same(sc.build_tile_labels({18: new[0]}), w.want(tiles, {18: new[1]}))
    _same(sc.build_tile_labels({18: w.hi[0]}), w.want(tiles, {18: w.hi[1]}))  # an older table under the new ranks
    sc.free()


def _err(fn, code, *words):
    with pytest.raises(OsmtError) as e:
        fn()
    assert e.value.code == code and all(x in str(e.value) for x in words), str(e.value)


def test_refusals_name_their_offender(gpu_ctx, shapes, tables):
    w, L, h = shapes, lib.load(), gpu_ctx._h
    sc = w.scene([(18, *w.spots[1]), (10, 0, 0)])
    _err(lambda: sc.build_tile_labels({18: w.hi[0]}), A.INVALID_ARG, "tile 1", "zoom 10", "no label bindings")
    _err(lambda: sc.build_tile_labels({18: w.hi[0], 10: w.hi[0]}), A.INVALID_ARG, "covers zooms 16..18")
    _err(lambda: sc.build_tile_labels({18: w.hi[0], 10: 1 << 20}), A.INVALID_ARG, "not registered")
    up = gpu_ctx.upload(__import__("osm_renderer_amd.synth", fromlist=["x"]).config2(1))
    _err(lambda: up.build_tile_labels({z: w.hi[0] for z in range(19)}), A.INVALID_ARG, "not built by osmt_scene_build_tiles")
    up.free()
    area = tl.string_labels([dict(chars="AB", font=tables[1].font_id, font_size=10.0, center=(50.0, 50.0))])
    area.job_label_off = np.array([0, 1, 1], np.uint32)
    both = {18: w.hi[0], 10: w.lo[0]}
    sb = area.as_batch()
    sb.chars = None  # a NULL pool with a non-zero count
    _err(lambda: lib.check(L.osmt_scene_build_tile_labels(h, sc._h, (C.c_uint32 * 19)(*[both.get(z, A.BINDINGS_NONE) for z in range(19)]), C.byref(sb))),
         A.INVALID_ARG, "area labels", "NULL")
    empty = labels.StringLabelList(area.labels[:0], [0, 0, 1], area.runs[:0], [], np.zeros((0, 2), np.int32), np.zeros((0, 2)))
    _err(lambda: sc.build_tile_labels(both, empty), A.INVALID_ARG, "job_label_off must run from 0 to n_labels")  # no labels, bad offsets
    area.job_label_off = np.array([0, 1, 0], np.uint32)
    _err(lambda: sc.build_tile_labels(both, area), A.INVALID_ARG, "job_label_off")
    sc.free()
    # the validators that ask the context
    gids = [n[0] for n in w.nodes]
    n_tiles = len(w.refs)

    def node_index(gid=w.gid, node_ids=gids, lists=None, first_off=0):
        d = styled.NodeIndex(node_ids, [[0]] * n_tiles if lists is None else lists)
        d.node_off[0] = first_off
        dd = d.as_desc()
        return lambda: lib.check(L.osmt_validate_node_index(C.byref(dd), gid, h)) or d

    _err(node_index(), A.INVALID_ARG, "node index already")  # a second registration
    _err(node_index(gid=1 << 20), A.INVALID_ARG, "is not registered")
    fresh = gpu_ctx.register_geodata(geodata_of(w.r))
    _err(node_index(gid=fresh), A.INVALID_ARG, "no tile index")
    gpu_ctx.register_tile_index(fresh, styled.TileIndex([(k, [], []) for k in sorted(w.refs)]))
    node_index(gid=fresh)()
    _err(node_index(gid=fresh, node_ids=gids[:-1]), A.INVALID_ARG, "n_nodes")
    _err(node_index(gid=fresh, first_off=1), A.INVALID_ARG, "node_off[0] is 1")
    _err(node_index(gid=fresh, lists=[[0]] * (n_tiles + 1)), A.INVALID_ARG, "node_off", "does not end")
    _err(node_index(gid=fresh, lists=[[len(gids)]] * n_tiles), A.INVALID_ARG, f"nodes[0] = {len(gids)}")
    _, font, _, ids = tables
    P = C.POINTER(A.LabelStyleRec)

    def style(**kw):
        st = tl.label_styles([kw])
        return lambda: lib.check(L.osmt_validate_label_styles(st.ctypes.data_as(P), 1, h)) or st

    style(icon=ids[0], font_size=10.0, font_id=font.font_id)()
    _err(style(icon=1 << 30), A.INVALID_ARG, "icon_image")
    _err(style(font_size=10.0, font_id=1 << 30), A.INVALID_ARG, "font_id")

    def bindings(rows, texts=TEXTS, gid=w.gid):
        b = styled.LabelBindings(gid, 0, 18, rows + [[]] * (len(gids) - len(rows)), texts)
        d = b.as_desc()
        return lambda: lib.check(L.osmt_validate_label_bindings(C.byref(d), h)) or b

    bindings([[(w.first, 0), (w.first + 1, None)]])()
    _err(bindings([[(1 << 30, 0)]]), A.INVALID_ARG, "not a registered label style")
    _err(bindings([[(w.first, len(TEXTS))]]), A.INVALID_ARG, "text pool")
    _err(bindings([[(w.first, 0)]], texts=[[0xD800]]), A.INVALID_ARG, "U+D800")
    _err(bindings([[(w.first, 0)]], gid=1 << 20), A.INVALID_ARG, "is not registered")
    _err(bindings([[(w.first, 0)]] * (len(gids) + 1)), A.INVALID_ARG, "node_off")


def test_limits_are_refused_with_the_exact_figure(gpu_ctx, shapes):
    w = shapes
    tile = (18, *w.spots[1])
    node = w.refs[tile[1:]][0][0]
    plain = 6  # neither icon nor text: 104 bytes per label and nothing else

    def table(k):
        rows = [[] for _ in range(node + 1)]
        rows[node] = [(plain, None)] * k
        return w.bind(rows, 18, 18)

    over, full = table(A.TILE_LABELS_MAX + 1), table(A.TILE_LABELS_MAX)
    sc = w.scene([(18, CX + 7, CY + 300), tile])
    _err(lambda: sc.build_tile_labels({18: over[0]}), A.UNSUPPORTED, "tile 1", "65537 node labels", "OSMT_TILE_LABELS_MAX")
    got = sc.build_tile_labels({18: full[0]})  # the limit itself builds, in the sort's device-memory tier
    assert np.diff(got.job_label_off).tolist() == [0, A.TILE_LABELS_MAX]
    _same(got, w.want([(18, CX + 7, CY + 300), tile], {18: full[1]}))
    sc.free()
    many = w.scene([tile] * (A.TILE_LABELS_MAX + 1))
    _err(lambda: many.build_tile_labels({18: full[0]}), A.UNSUPPORTED, f"{(1 << 32) + 65536} node labels")
    _same(many.build_tile_labels({18: w.hi[0]}), w.want([tile] * (A.TILE_LABELS_MAX + 1), {18: w.hi[1]}))  # and a correct build behind it
    many.free()


# ---- pixels ---------------------------------------------------------------------------------------------------------
Z = 16
TX, TY = CX >> 2, CY >> 2


@pytest.fixture(scope="module")
def town(gpu_ctx, tables, tmp_path_factory):
    """10 x 7 tiles of zoom 16 with four labelled nodes and a filled square each"""
    rng = np.random.default_rng(41)
    nodes, refs, bind, ways = [], {}, [], []

    def node(fx, fy, index=True):
        lat, lon = tl.latlon_of(Z, fx, fy)
        nodes.append((int(rng.integers(1, 1 << 60)), lat, lon))
        if index:
            refs.setdefault((int(fx * 4), int(fy * 4)), []).append(len(nodes) - 1)
        return len(nodes) - 1

    spots = [(0.25, 0.25), (0.7, 0.3), (0.3, 0.72), (0.72, 0.75)]
    kinds = [[(2, 2)], [(4, 0), (1, None)], [(0, 4)], [(7, 2), (3, 0)]]
    for j in range(7):
        for i in range(10):
            for (fx, fy), b in zip(spots, kinds):
                node(TX + i + fx + 0.02 * rng.random(), TY + j + fy + 0.02 * rng.random())
                bind.append(b)
    for j in range(7):
        for i in range(10):
            sq = [node(TX + i + a, TY + j + b, index=False) for a, b in ((0.4, 0.4), (0.6, 0.4), (0.6, 0.6), (0.4, 0.6))]
            ways.append((int(rng.integers(1, 1 << 60)), sq + [sq[0]]))
            bind += [[]] * 4
    for k in list(refs):
        refs.setdefault(k, [])
    w = World(gpu_ctx, tables, tmp_path_factory.mktemp("tl") / "town.bin", nodes, refs, ways)
    w.all = w.bind(bind)
    yield w
    w.close()


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
    w = town
    tiles = [(Z, TX + k % 10, TY + k // 10) for k in range(n_tiles)]
    ids, mir = {Z: w.all[0]}, {Z: w.all[1]}
    sc = w.scene(tiles, scale)
    got = sc.build_tile_labels(ids)
    want = w.want(tiles, mir, scale)
    _same(got, want)
    assert len(want.labels) >= 6 * n_tiles
    out = gpu_ctx.render(sc).cpu().numpy()
    st = sc.label_status()
    sc.set_string_labels(want)
    assert np.array_equal(gpu_ctx.render(sc).cpu().numpy(), out) and np.array_equal(sc.label_status(), st)
    sub = list(range(n_tiles)) if n_tiles <= 5 else list(range(0, n_tiles, 9))
    ll = _oracle_labels(want.subset(sub), tables)  # the host expansion of the compared tiles only: it is Python
    ref, rst = oracle.render_batch(_latlon(sc.dl).subset(sub), images=_images(tables), threads=min(8, len(sub)), labels=ll, want_status=True)
    lab_sub = np.concatenate([np.arange(int(want.job_label_off[i]), int(want.job_label_off[i + 1])) for i in sub])
    assert np.array_equal(st[lab_sub], rst) and rst.sum() > 0
    assert np.array_equal(out[sub], ref)
    # area labels in front: a centred text on top of the first node of every tile (that node loses), a text along a way
    font = tables[1].font_id
    parts, under = [], []
    for t in range(n_tiles):
        mine = want.labels[int(want.job_label_off[t]) : int(want.job_label_off[t + 1])]
        a = int(np.nonzero((mine["has_icon"] == 1) & (mine["image_id"] == tables[3][0]))[0][0])  # the node with the 16 x 16 icon
        under.append(a)
        cx, cy = float(mine[a]["icon_center_x"]), float(mine[a]["icon_center_y"])
        way = [(int(20 * scale + 12 * scale * k), int(128 * scale + (k % 2))) for k in range(12)]
        parts.append(tl.string_labels([dict(chars="DDDD", font=font, font_size=12.0 * scale, center=(cx, cy), color=(90, 0, 0)),
                                    dict(chars="ABCDE", font=font, font_size=9.0 * scale, position=A.TEXT_LINE, pts=way)]))
    area = labels.concat_string_labels(parts)
    sc.build_tile_labels(ids, area)
    both = labels.splice_string_labels(area, want)
    out2 = gpu_ctx.render(sc).cpu().numpy()
    st2 = sc.label_status()
    ll2 = _oracle_labels(both.subset(sub), tables)
    ref2, rst2 = oracle.render_batch(_latlon(sc.dl).subset(sub), images=_images(tables), threads=min(8, len(sub)), labels=ll2, want_status=True)
    pos, node_st = 0, []
    for i in sub:  # on the oracle first: per tile the node labels behind its two area labels
        n = int(both.job_label_off[i + 1] - both.job_label_off[i])
        node_st += rst2[pos + 2 : pos + n].tolist()
        assert rst2[pos] == 1  # the area label itself is placed
        assert rst2[pos + 2 + under[i]] == 0  # the node under it loses the collision
        pos += n
    assert 0 in node_st and 1 in node_st
    lab_sub2 = np.concatenate([np.arange(int(both.job_label_off[i]), int(both.job_label_off[i + 1])) for i in sub])
    assert np.array_equal(st2[lab_sub2], rst2) and np.array_equal(out2[sub], ref2)
    sc.set_string_labels(both)  # the host-spliced batch
    assert np.array_equal(gpu_ctx.render(sc).cpu().numpy(), out2) and np.array_equal(sc.label_status(), st2)
    sc.free()
