"""Area labels of tile-built scenes, the parts that need no GPU: the layouts of the new ABI records, the validator refusals that
need no device, the host mirror osmt::area_labels_of_tile (osm_renderer_amd/host/osmt_arealabels.hpp) against a Python
restatement written from the reference alone that does LITERALLY sort, sort, merge (tests/_arealabels.order_literal) over a
few thousand seeded cases of random styles with many ties and global ids at the extremes, the claim the device's order rests
on — a tile's multipolygon elements numbered in front of its way elements and ONE sort by (rank, global id, number) is that
sort, sort, merge — against the same restatement, and the mirror in a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from osm_renderer_amd import abi, labels, lib, styled
from tests import _anchors as an
from tests import _arealabels as al
from tests import _tilelabels as tl
from tests._styled_feed import geodata_of
from tests._tilequery import center_z18

A = abi
MP = al.MP
CX, CY = center_z18()
TEXTS = ["ABC", "", "Арбатская", [0x10FFFF, 0x20, 0x4E00]]
GIDS = [0, 1 << 32, (1 << 64) - 1, 77, 78]  # 77: a way and a multipolygon share it


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _refused(rc, code, *words):
    msg = lib.load().osmt_last_error().decode()
    assert rc == code and all(w in msg for w in words), (rc, msg)


def test_layouts_match_the_header():
    s = al.shim().al_sizeof
    assert s(0) == C.sizeof(A.AreaLabelBindingsDesc) == 88 and s(10) == A.AreaLabelBindingsDesc.way_off.offset
    assert s(11) == A.AreaLabelBindingsDesc.n_chars.offset
    assert s(1) == C.sizeof(A.AreaAnchor) == labels.AREA_ANCHOR_DTYPE.itemsize == 32
    assert s(12) == A.AreaAnchor.status.offset == labels.AREA_ANCHOR_DTYPE.fields["status"][1]


def test_validators_without_a_context():
    L = lib.load()
    d = styled.AreaLabelBindings(0, 3, 9, [[(0, None)]], [[]], []).as_desc()
    _refused(L.osmt_validate_area_label_bindings(C.byref(d), None), A.INVALID_ARG, "geodata id 0", "no context")
    for lo, hi in ((9, 3), (0, 19)):
        d = styled.AreaLabelBindings(0, lo, hi, [[]], [], []).as_desc()
        _refused(L.osmt_validate_area_label_bindings(C.byref(d), None), A.INVALID_ARG, "zoom range")
    _refused(L.osmt_validate_area_label_bindings(None, None), A.INVALID_ARG, "NULL")
    out = C.c_uint32()
    _refused(L.osmt_register_area_label_bindings(None, C.byref(d), C.byref(out)), A.INVALID_ARG, "NULL")
    _refused(L.osmt_scene_build_tile_labels_all(None, None, None, None, None, 0), A.INVALID_ARG, "ctx")
    n = C.c_size_t()
    _refused(L.osmt_scene_read_declined_anchors(None, None, None, 0, C.byref(n)), A.INVALID_ARG, "NULL")
    _refused(L.osmt_scene_read_tile_area_labels(None, None, None, None, None, None, None, None, None, None), A.INVALID_ARG, "NULL")


TILES = [(18, CX, CY), (18, CX + 1, CY), (18, CX + 2, CY), (17, CX >> 1, CY >> 1), (15, CX >> 3, CY >> 3), (12, (CX + 40) >> 6, CY >> 6), (0, 0, 0),
         (18, CX + 40, CY + 3), (18, CX + 300, CY)]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    w = al.feature_world((CX, CY), GIDS)
    r, refs = w.write(tmp_path_factory.mktemp("area_labels") / "areas.bin")
    yield w, r, refs
    r.close()


def _random_styles(rng, n):
    rows = []
    for _ in range(n):
        row = dict(layer=[None, 0, 1, -1][int(rng.integers(0, 4))], z_index=[-0.0, 0.0, 1.5][int(rng.integers(0, 3))])
        if rng.random() < 0.4:
            row["icon"] = int(rng.integers(0, 4))
        if rng.random() < 0.8:
            row["text_style"] = True
            if rng.random() < 0.85:
                row["font_size"] = float(rng.integers(6, 20))
            if rng.random() < 0.5:
                row["text_color"] = tuple(int(v) for v in rng.integers(0, 256, 3))
        row["text_position"] = int(rng.integers(0, 3))
        rows.append(row)
    return tl.label_styles(rows), [int(rng.integers(0, 40)) for _ in rows]


def _random_bindings(rng, n, n_styles):
    return [[(int(rng.integers(0, n_styles)), None if rng.random() < 0.2 else int(rng.integers(0, len(TEXTS)))) for _ in range(int(rng.integers(0, 4)))]
            for _ in range(n)]


def _random_positions(rng, n):
    pos = np.zeros(n, labels.LABEL_POSITION_DTYPE)
    pos["status"] = rng.choice([A.LABEL_OK, A.LABEL_OK, A.LABEL_NONE], n)
    pos["x"], pos["y"] = rng.uniform(-300, 600, n), rng.uniform(-300, 600, n)
    return pos


def test_mirror_equals_the_literal_restatement_and_one_sort_is_that_order(world):
    w, r, refs = world
    n_labels = n_line = n_none = ties = 0
    for seed in range(2500):
        rng = np.random.default_rng(seed)
        st, icon_h = _random_styles(rng, 6)
        wb, mb = _random_bindings(rng, r.n_ways, len(st)), _random_bindings(rng, r.n_multipolygons, len(st))
        zoom, x, y = TILES[seed % len(TILES)]
        scale = 1 + seed % 2
        pts = rng.integers(-4000, 4000, (r.n_nodes, 2)).astype(np.int32)
        if seed % 3 == 0:
            pts[:, 0] = rng.integers(0, 3, r.n_nodes)  # many first.x == last.x
        wp, mpos = _random_positions(rng, r.n_ways), _random_positions(rng, r.n_multipolygons)
        W, M = al.elements(refs, w.mp_polygon_counts(), wb, mb, zoom, x, y)
        order = al.order_literal(W, M, st, w.way_gids(), w.mp_gids())
        assert al.order_one_sort(W, M, st, w.way_gids(), w.mp_gids()) == order, seed
        anchor = lambda e: (lambda p: (int(p["status"]), float(p["x"]), float(p["y"])))(mpos[e & ~MP] if e & MP else wp[e])
        want = al.records(order, TEXTS, st, icon_h, scale, lambda i: w.ways[i][1], lambda n: pts[n], anchor)
        m = al.Mirror(r, wb, mb, TEXTS)
        got = m.labels(st, icon_h, zoom, x, y, scale, pts, wp, mpos)
        m.close()
        for g, v, name in zip(got, want, ("labels", "runs", "chars", "way_pts", "way_sincos")):
            assert g.shape == v.shape and np.array_equal(_u8(g), _u8(v)), (seed, name)
        n_labels += len(order)
        n_line += int((want[1]["position"] == A.TEXT_LINE).sum())
        n_none += sum(1 for l, (mp, e, s, t) in zip(want[0], order) if st[s]["has_icon"] and not l["has_icon"])
        keys = [(al._key(st, w.mp_gids() if e[0] else w.way_gids())(e[1:])) for e in order]
        ties += sum(1 for a, b in zip(keys, keys[1:]) if a == b)
    assert n_labels > 20000 and n_line > 2000 and n_none > 500 and ties > 2000, (n_labels, n_line, n_none, ties)


def test_equal_keys_across_kinds_put_the_multipolygon_first(world):
    w, r, refs = world
    st = tl.label_styles([dict(font_size=10.0), dict(layer=0, z_index=-0.0, font_size=12.0)])  # None vs Some(0), +0.0 vs -0.0: one rank
    wb, mb = [[] for _ in range(r.n_ways)], [[] for _ in range(r.n_multipolygons)]
    wb[4] = [(1, 0), (0, 0), (1, 1)]  # way 4 and multipolygon 0 share global id 77
    mb[0] = [(0, 0), (1, 0)]
    W, M = al.elements(refs, w.mp_polygon_counts(), wb, mb, 18, CX, CY)
    order = al.order_literal(W, M, st, w.way_gids(), w.mp_gids())
    assert order == [(True, 0, 0, 0), (True, 0, 1, 0), (False, 4, 1, 0), (False, 4, 0, 0), (False, 4, 1, 1)]
    assert al.order_one_sort(W, M, st, w.way_gids(), w.mp_gids()) == order


@pytest.mark.parametrize("scale", [1, 2, 3, 4])
def test_mirror_with_the_hosts_libm_and_anchors(world, scale):
    """the defaults of the mirror — project_libm and osmt::HostAnchors — against Python floats and the anchors' own mirror"""
    w, r, refs = world
    rng = np.random.default_rng(3)
    st, icon_h = _random_styles(rng, 8)
    wb, mb = _random_bindings(rng, r.n_ways, len(st)), _random_bindings(rng, r.n_multipolygons, len(st))
    g = geodata_of(r)
    f = an.mercator_factors(r.node_table())
    m = al.Mirror(r, wb, mb, TEXTS)
    seen = 0
    for zoom, x, y in TILES:
        def anchor(e):
            p = an.mirror_position(g, f, e, zoom, x, y, scale)
            return int(p["status"]), float(p["x"]), float(p["y"])

        W, M = al.elements(refs, w.mp_polygon_counts(), wb, mb, zoom, x, y)
        order = al.order_literal(W, M, st, w.way_gids(), w.mp_gids())
        want = al.records(order, TEXTS, st, icon_h, scale, lambda i: w.ways[i][1],
                          lambda n: tl.py_project(w.nodes[n][1], w.nodes[n][2], zoom, x, y, scale), anchor)
        got = m.labels(st, icon_h, zoom, x, y, scale)
        for a, b, name in zip(got, want, ("labels", "runs", "chars", "way_pts", "way_sincos")):
            assert a.shape == b.shape and np.array_equal(_u8(a), _u8(b)), (zoom, x, y, name)
        seen += len(order)
    assert seen > 60
    m.close()


def test_mirror_under_sanitizers(world, tmp_path):
    """the fixed styles and binding rule of tests/arealabels_host_main.cpp, restated here"""
    w, r, refs = world
    st = tl.label_styles([dict(font_size=11.5), dict(layer=0, z_index=-0.0, icon=3), dict(layer=-1, font_size=9.0, text_position=A.LABEL_POSITION_LINE),
                          dict(z_index=2.5, font_size=14.0, text_color=(200, 10, 30), text_position=A.LABEL_POSITION_CENTER), dict(icon=1, font_size=8.0)])
    icon_h = [0, 7, 0, 0, 16]
    texts = ["ABC", ""]
    rule = lambda n: [[((i + k) % 5, None if k % 2 else i % 2) for k in range(i % 4)] for i in range(n)]
    wb, mb = rule(r.n_ways), rule(r.n_multipolygons)
    path = str(tmp_path / "w.bin")
    al.write_geodata(path, w.nodes, w.ways, w.polygons, w.mps, tile_refs=refs)
    tiles = TILES[:7]
    out = subprocess.run([al.build_host_main(), path, "2"] + [str(v) for t in tiles for v in t], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert lines[0] == f"bindings {sum(len(b) for b in wb)} {sum(len(b) for b in mb)} 2 3"
    g, f = geodata_of(r), an.mercator_factors(r.node_table())
    k, seen = 1, 0
    for zoom, x, y in tiles:
        def anchor(e):
            p = an.mirror_position(g, f, e, zoom, x, y, 2)
            return int(p["status"]), float(p["x"]), float(p["y"])

        W, M = al.elements(refs, w.mp_polygon_counts(), wb, mb, zoom, x, y)
        order = al.order_literal(W, M, st, w.way_gids(), w.mp_gids())
        lab, runs, chars, pts, scs = al.records(order, texts, st, icon_h, 2, lambda i: w.ways[i][1],
                                                lambda n: tl.py_project(w.nodes[n][1], w.nodes[n][2], zoom, x, y, 2), anchor)
        assert lines[k] == f"tile {zoom} {x} {y} {len(lab)} {len(chars)} {len(pts)}"
        k += 1
        for l, s in zip(lab, runs):
            got = lines[k].split()
            want = [l["has_icon"], l["has_text"], l["image_id"], l["seg_off"], l["n_segs"], s["y_offset"], s["position"], s["pt_off"], s["n_pts"]]
            assert [int(v) for v in got[:9]] == [int(v) for v in want] and [int(v) for v in got[12:]] == l["text_color"].tolist()
            assert [float(v) for v in got[9:12]] == [float(s["font_size"]), float(l["icon_center_x"]), float(l["icon_center_y"])]
            k += 1
        for p, sc in zip(pts, scs):
            got = lines[k].split()
            assert got[0] == "pt" and [int(got[1]), int(got[2])] == p.tolist() and [float(got[3]), float(got[4])] == sc.tolist()
            k += 1
        seen += len(lab)
    assert k == len(lines) and seen > 20
