"""The osm_ids filter, the parts that need no GPU: the validator rules that need no context, the sort / dedup step of a
registration and the host twin of the plane kernel (osm_renderer_amd/host/osmt_idfilter.hpp) against numpy, and the three host
twins — osmt::styled_areas_of_tile, osmt::node_labels_of_tile, osmt::area_labels_of_tile — with their osm_ids argument against
the Python restatements of the unfiltered queries (tests/_tilequery.py, tests/_tilelabels.py, tests/_arealabels.py) with
filter_entities_by_ids (reader.rs:254-262) applied where the reference applies it: LAST in the query, on the sorted unique
entity lists, behind the drop of the multipolygons without polygons and in front of every style.  The twins and the sort / dedup
step run once more in a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from osm_renderer_amd import abi, labels, lib
from tests import _arealabels as al
from tests import _idfilter as idf
from tests import _tilelabels as tl
from tests import _tilequery as tq
from tests._tilequery import center_z18

A = abi
MP = al.MP
CX, CY = center_z18()
TEXTS = ["ABC", "", "Арбатская"]
GIDS = [0, 1 << 32, (1 << 64) - 1, 77, 78]  # 77: way 4, multipolygon 0 and node 5 share it
TILES = [(18, CX, CY), (18, CX + 1, CY), (17, CX >> 1, CY >> 1), (12, (CX + 40) >> 6, CY >> 6), (0, 0, 0), (18, CX + 40, CY + 3), (18, CX + 300, CY)]


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _refused(rc, code, *words):
    msg = lib.load().osmt_last_error().decode()
    assert rc == code and all(w in msg for w in words), (rc, msg)


def test_exports_and_validators_without_a_context():
    L = lib.load()
    for name in ("osmt_validate_id_filter", "osmt_register_id_filter", "osmt_read_id_filter", "osmt_scene_build_tiles_filtered"):
        assert name in lib.EXPORTS and hasattr(L, name)
    assert A.ID_FILTER_NONE == 0xFFFFFFFF
    one = (C.c_uint64 * 1)(5)
    _refused(L.osmt_validate_id_filter(one, 1 << 31, 0, None), A.INVALID_ARG, str(1 << 31), "2^31")  # judged before the array is read
    _refused(L.osmt_validate_id_filter(None, 3, 0, None), A.INVALID_ARG, "NULL", "n = 3")
    _refused(L.osmt_validate_id_filter(one, 1, 5, None), A.INVALID_ARG, "geodata id 5", "no context")
    _refused(L.osmt_validate_id_filter(None, 0, 6, None), A.INVALID_ARG, "geodata id 6", "no context")  # an empty set is a set: only the file is missing
    out = C.c_uint32()
    _refused(L.osmt_register_id_filter(None, 0, one, 1, C.byref(out)), A.INVALID_ARG, "NULL")
    n = (C.c_size_t * 3)()
    _refused(L.osmt_read_id_filter(None, 0, None, None, None, None, n), A.INVALID_ARG, "NULL")
    _refused(L.osmt_scene_build_tiles_filtered(None, None, 0, None), A.INVALID_ARG, "NULL")


EDGE_IDS = [0, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1, (7 << 32) | 5, (7 << 32) | 6, (8 << 32) | 5]  # pairs one word apart


def test_sort_dedup_and_the_planes_host_twin():
    rng = np.random.default_rng(5)
    assert idf.host_set([]).tolist() == [] and idf.host_set([9, 9, 9]).tolist() == [9]
    pool = np.array(EDGE_IDS + rng.integers(0, 1 << 63, 300, dtype=np.uint64).tolist(), dtype=np.uint64)
    for n_ent in (0, 1, 63, 64, 65, 255, 256, 257, 1000):
        gids = rng.choice(pool, n_ent) if n_ent else np.zeros(0, np.uint64)
        for n_ids in (0, 1, 2, 1000):
            ids = rng.choice(pool, n_ids) if n_ids else np.zeros(0, np.uint64)  # any order, with repeats
            assert idf.host_set(ids).tolist() == np.unique(ids).tolist()
            got, want = idf.host_plane(gids, ids), idf.numpy_plane(gids, ids)
            assert len(got) == (n_ent + 63) // 64 * 2 and np.array_equal(got, want), (n_ent, n_ids)
    # a compare of one 32-bit half alone would take these for each other
    assert idf.host_plane([(7 << 32) | 5, (7 << 32) | 6, (8 << 32) | 5, 5], [(7 << 32) | 5]).tolist() == [1, 0]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """tests._arealabels.feature_world with its nodes listed in index tiles too, one of them under the shared global id"""
    w = al.feature_world((CX, CY), GIDS)
    w.nodes[5] = (77,) + tuple(w.nodes[5][1:])
    spots = [(CX, CY), (CX + 1, CY), (CX + 40, CY + 3)]
    for i in range(len(w.nodes)):
        w.refs.setdefault(spots[i % 3], ([], [], []))[0].append(i)
        if i % 5 == 0:
            w.refs.setdefault(spots[(i + 1) % 3], ([], [], []))[0].append(i)  # listed twice: a repeat the query removes
    path = str(tmp_path_factory.mktemp("idfilter") / "world.bin")
    r, refs = w.write(path)
    yield w, r, refs, path
    r.close()


def _filters(w, rng):
    every = [n[0] for n in w.nodes] + w.way_gids() + w.mp_gids()
    some = [int(v) for v in rng.choice(np.array(every, dtype=np.uint64), len(every) // 2, replace=False)]
    return {
        "none": None,
        "empty": [],
        "every id": every,
        "any order, repeats": [int(v) for v in rng.permutation(np.array(some + some[:7], dtype=np.uint64))],
        "the shared id": [77],
        "a multipolygon without polygons": [11, 902, 900],
        "unknown ids": [123456789, (1 << 64) - 2],
    }


def _rule(n, n_styles):
    """entity i: i % 4 bindings, binding k: style (i + k) % n_styles, text none for odd k, else i % 2 — the rule of the host programs"""
    return [[((i + k) % n_styles, None if k % 2 else i % 2) for k in range(i % 4)] for i in range(n)]


def _label_styles():
    st = tl.label_styles([dict(font_size=11.5), dict(layer=0, z_index=-0.0, icon=3), dict(layer=-1, font_size=9.0, text_position=A.LABEL_POSITION_LINE),
                          dict(z_index=2.5, font_size=14.0, text_position=A.LABEL_POSITION_CENTER), dict(icon=1, font_size=8.0)])
    return st, [0, 7, 0, 0, 16]


def _draw_rule(w):
    """tests/tilequery_host_main.cpp: way i: i % 3 styles, falling ids; multipolygon m: (m + 1) % 3 styles"""
    return ([[7 * i + 5 - k for k in range(i % 3)] for i in range(len(w.ways))], [[11 * m + 9 - k for k in range((m + 1) % 3)] for m in range(len(w.mps))])


def _restated(w, refs, flt, ws, ms, nb, wb, mb, st, icon_h, texts, zoom, x, y, scale, point_of, anchor):
    """the three results of one tile with the filter applied last in the query: areas as pairs, node records, area records"""
    keep = (lambda gid: True) if flt is None else (lambda gid, s=set(flt): gid in s)
    areas, _, _ = tq.restate(refs, w.mp_polygon_counts(), ws, ms, zoom, x, y)
    areas = [(e, s) for e, s in areas if keep(w.mp_gids()[e & ~MP] if e & MP else w.way_gids()[e])]
    ngids = [n[0] for n in w.nodes]
    nodes = tl.restate(refs, ngids, [b if keep(ngids[i]) else [] for i, b in enumerate(nb)], texts, st, icon_h, zoom, x, y, scale, point_of)
    W, M = al.elements(refs, w.mp_polygon_counts(), wb, mb, zoom, x, y)
    W, M = [e for e in W if keep(w.way_gids()[e[0]])], [e for e in M if keep(w.mp_gids()[e[0]])]
    order = al.order_literal(W, M, st, w.way_gids(), w.mp_gids())
    return areas, nodes, al.records(order, texts, st, icon_h, scale, lambda i: w.ways[i][1], point_of, anchor), order


def test_the_twins_filter_last(world):
    w, r, refs, _ = world
    rng = np.random.default_rng(11)
    st, icon_h = _label_styles()
    ws, ms = _draw_rule(w)
    nb, wb, mb = _rule(r.n_nodes, 4), _rule(r.n_ways, 5), _rule(r.n_multipolygons, 5)
    wb[4], mb[0], ms[1] = [(0, 0), (1, None)], [(3, 0)], [3]  # the sharers of global id 77 have labels; the multipolygon without polygons has a style
    tqm, tlm, alm = tq.Mirror(r, ws, ms), tl.Mirror(r, nb, TEXTS), al.Mirror(r, wb, mb, TEXTS)
    pts = rng.integers(-4000, 4000, (r.n_nodes, 2)).astype(np.int32)
    wp, mpos = np.zeros(r.n_ways, labels.LABEL_POSITION_DTYPE), np.zeros(r.n_multipolygons, labels.LABEL_POSITION_DTYPE)
    for pos in (wp, mpos):
        pos["status"] = rng.choice([A.LABEL_OK, A.LABEL_OK, A.LABEL_NONE], len(pos))
        pos["x"], pos["y"] = rng.uniform(-300, 600, len(pos)), rng.uniform(-300, 600, len(pos))
    anchor = lambda e: (lambda p: (int(p["status"]), float(p["x"]), float(p["y"])))(mpos[e & ~MP] if e & MP else wp[e])
    seen = {}
    for name, flt in _filters(w, rng).items():
        n_a = n_n = n_l = 0
        for zoom, x, y in TILES:
            scale = 1 + (x + zoom) % 2
            areas, nodes, recs, order = _restated(w, refs, flt, ws, ms, nb, wb, mb, st, icon_h, TEXTS, zoom, x, y, scale, lambda n: pts[n], anchor)
            assert tq.pairs(idf.areas(tqm, zoom, x, y, flt)) == areas, (name, zoom, x, y)
            got = idf.node_labels(tlm, st, icon_h, zoom, x, y, scale, pts, flt)
            for g, v, what in zip(got, nodes, ("labels", "runs", "chars")):
                assert g.shape == v.shape and np.array_equal(_u8(g), _u8(v)), (name, zoom, x, y, what)
            got, asked = idf.area_labels(alm, st, icon_h, zoom, x, y, scale, pts, wp, mpos, flt, want_asked=True)
            for g, v, what in zip(got, recs, ("labels", "runs", "chars", "way_pts", "way_sincos")):
                assert g.shape == v.shape and np.array_equal(_u8(g), _u8(v)), (name, zoom, x, y, what)
            assert asked <= len(order)  # an entity the filter removed is never asked for an anchor
            assert (1 | MP) not in [e for e, _ in areas]  # global id 11: listed or not, it has no polygons
            if flt is None:  # the default argument is the twin as it was
                assert tq.pairs(tqm.areas(zoom, x, y)) == areas
                assert all(np.array_equal(_u8(a), _u8(b)) for a, b in zip(tlm.labels(st, icon_h, zoom, x, y, scale, pts), nodes))
                assert all(np.array_equal(_u8(a), _u8(b)) for a, b in zip(alm.labels(st, icon_h, zoom, x, y, scale, pts, wp, mpos), recs))
            n_a, n_n, n_l = n_a + len(areas), n_n + len(nodes[0]), n_l + len(recs[0])
        seen[name] = (n_a, n_n, n_l)
    for m in (tqm, tlm, alm):
        m.close()
    assert seen["empty"] == (0, 0, 0) and seen["unknown ids"] == (0, 0, 0)
    assert seen["every id"] == seen["none"] and min(seen["none"]) > 40
    assert all(0 < a < b for a, b in zip(seen["any order, repeats"], seen["none"]))
    # one set serves the three kinds: the shared id keeps the node, the way and the multipolygon, each with its own bindings
    assert all(v > 0 for v in seen["the shared id"])
    # multipolygon 1 (global id 11) has no polygons: listing it does not bring it back; 900 and 902 are a way and a multipolygon
    a, n, l = seen["a multipolygon without polygons"]
    assert a > 0 and n == 0 and l > 0


def test_the_twins_and_the_sort_under_sanitizers(world):
    """tests/idfilter_host_main.cpp, built with -fsanitize=address,undefined and run directly: the binding rules are restated here"""
    w, r, refs, path = world
    st, icon_h = _label_styles()
    ws, ms = _draw_rule(w)
    nb, wb, mb = _rule(r.n_nodes, 4), _rule(r.n_ways, 5), _rule(r.n_multipolygons, 5)
    texts = ["ABC", ""]
    ngids = [n[0] for n in w.nodes]
    exe = idf.build_host_main()
    from tests import _anchors as an
    from tests._styled_feed import geodata_of

    g, f = geodata_of(r), an.mercator_factors(r.node_table())
    rng = np.random.default_rng(2)
    total = 0
    for name, flt in _filters(w, rng).items():
        args = ["-1"] if flt is None else [str(len(flt))] + [str(v) for v in flt]
        out = subprocess.run([exe, path, "2"] + args + [str(v) for t in TILES for v in t], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (name, out.stderr[-2000:])
        lines = out.stdout.splitlines()
        ids = flt or []
        assert lines[0].split() == ["set", str(len(set(ids)))] + [str(v) for v in sorted(set(ids))]
        for line, kind, gids in zip(lines[1:4], ("ways", "multipolygons", "nodes"), (w.way_gids(), w.mp_gids(), ngids)):
            want = idf.numpy_plane(gids, ids)
            assert line.split() == ["plane", kind, str(len(want))] + [f"{int(v):08x}" for v in want], (name, kind)
        k = 4
        for zoom, x, y in TILES:
            def anchor(e):
                p = an.mirror_position(g, f, e, zoom, x, y, 2)
                return int(p["status"]), float(p["x"]), float(p["y"])

            point_of = lambda n: tl.py_project(w.nodes[n][1], w.nodes[n][2], zoom, x, y, 2)
            areas, nodes, recs, order = _restated(w, refs, flt, ws, ms, nb, wb, mb, st, icon_h, texts, zoom, x, y, 2, point_of, anchor)
            assert lines[k].split() == ["areas", str(len(areas))] + [f"{e}:{s}" for e, s in areas], (name, zoom, x, y)
            assert lines[k + 1] == f"nodes {len(nodes[0])} {len(nodes[2])}", (name, zoom, x, y)
            asked = sum(1 for mp, e, s, t in order
                        if st[s]["has_icon"] or (st[s]["has_text_style"] and st[s]["has_font_size"] and t is not None and
                                                 not ((not mp) if st[s]["text_position"] == A.LABEL_POSITION_NONE else st[s]["text_position"] == A.LABEL_POSITION_LINE)))
            assert lines[k + 2] == f"arealabels {len(recs[0])} {len(recs[2])} {len(recs[3])} {asked}", (name, zoom, x, y)
            k += 3
            total += len(areas) + len(nodes[0]) + len(recs[0])
        assert k == len(lines)
    assert total > 300
