"""Node labels of tile-built scenes, the host side (no GPU): the layouts of the new records, the validator rules that need no
registered table, and the host mirror osmt::node_labels_of_tile (osm_renderer_amd/host/osmt_tilelabels.hpp) against a Python
restatement written from the reference alone (tests/_tilelabels.restate) on sparse indices at zooms 0, 10, 15 and 18, with the
ties that decide the order: layer None against Some(0), -0.0 against +0.0 z_index, two styles of one node with equal keys
(push order must survive the sort), global ids 0, 2^32, 2^63 and 2^64 - 1.  The mirror also runs in a stand-alone program under
AddressSanitizer and UBSan, and its libm projection is held against the oracle's on seeded nodes.  The validator rules that
ask a context for its tables are in tests/test_gpu_tile_labels.py: a context needs a device."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from osm_renderer_amd import abi, lib, styled
from tests import _tilelabels as tl
from tests._tilequery import center_z18

CX, CY = center_z18()
GIDS = [0, 1 << 32, 1 << 63, (1 << 64) - 1]
TEXTS = ["ABC", "", "Арбатская", [0x10FFFF, 0x20, 0x4E00]]
A = abi


def _styles():
    return tl.label_styles([
        dict(font_size=11.5),                                                # 0: layer None, z +0.0
        dict(layer=0, z_index=-0.0, icon=3),                                 # 1: Some(0), -0.0: ties with 0
        dict(icon=1, font_size=8.0, text_color=(9, 8, 7)),                   # 2: equal keys to 0 and 1, other content
        dict(layer=-1, font_size=9.0, text_position=A.LABEL_POSITION_LINE),  # 3: sorts first; Line on a node draws no text
        dict(z_index=2.5, font_size=14.0, text_color=(200, 10, 30), text_position=A.LABEL_POSITION_CENTER),
        dict(layer=1, text_style=True),                                      # 5: a text style without a font size
        dict(layer=1, z_index=-3.0),                                         # 6: neither icon nor text: still a record
    ])


ICON_H = [0, 7, 16, 0, 0, 0, 0]  # per style; 7: an odd height


def _world(tmp_path, seed=5, n=48):
    """n nodes in a sparse index: a cluster around (CX, CY), tiles 1, 8 and 300 tiles away, the four corners of the world;
    every node sits in one or two index tiles, in any order"""
    rng = np.random.default_rng(seed)
    spots = [(CX + dx, CY + dy) for dx in (-9, -8, -1, 0, 1, 7, 8, 300) for dy in (-8, -1, 0, 1, 8)]
    spots += [(0, 0), (0, tl.WORLD - 1), (tl.WORLD - 1, 0), (tl.WORLD - 1, tl.WORLD - 1)]
    gids = GIDS + [int(g) for g in rng.integers(1, 1 << 62, n - len(GIDS))]
    gids = [gids[i] for i in rng.permutation(n)]  # local id order is not global id order
    nodes, refs = [], {}
    for i in range(n):
        tx, ty = spots[int(rng.integers(0, len(spots)))] if i >= 8 else (CX, CY)
        lat, lon = tl.latlon_of(18, tx + rng.random(), ty + rng.random())
        nodes.append((gids[i], lat, lon))
        refs.setdefault((tx, ty), []).append(i)
        if i % 5 == 0:  # also listed by a neighbour: the query must not count it twice
            refs.setdefault((min(tx + 1, tl.WORLD - 1), ty), []).append(i)
    r, written = tl.make_world(tmp_path / "nodes.bin", nodes, refs)
    n_st = len(_styles())
    bind = []
    for i in range(n):
        k = (0, 1, 3, 2)[i % 4]
        b = [(int(s), None if (i + j) % 3 == 0 else int((i + j) % len(TEXTS))) for j, s in enumerate(rng.choice(n_st, k, replace=False))]
        bind.append(b)
    bind[0] = [(2, 0), (0, 2), (1, 1)]  # equal keys in falling and rising style id: push order decides
    bind[1] = [(1, 0), (0, None), (2, 3)]
    return r, written, gids, nodes, bind


TILES = [(18, CX, CY), (18, CX + 1, CY), (18, CX + 7, CY - 8), (15, CX >> 3, CY >> 3), (15, (CX >> 3) + 1, CY >> 3), (10, CX >> 8, CY >> 8), (0, 0, 0),
         (18, 0, 0), (18, tl.WORLD - 1, tl.WORLD - 1), (10, 0, 1023), (10, 1023, 0), (18, CX + 100, CY)]


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_layouts_match_the_header():
    s = tl.shim().tl_sizeof
    assert s(0) == C.sizeof(A.NodeIndexDesc) and s(10) == A.NodeIndexDesc.n_node_refs.offset
    assert s(1) == C.sizeof(A.LabelStyleRec) == styled.LABEL_STYLE_REC_DTYPE.itemsize == 48
    assert s(11) == A.LabelStyleRec.has_layer.offset == styled.LABEL_STYLE_REC_DTYPE.fields["has_layer"][1]
    assert s(12) == A.LabelStyleRec.text_position.offset == styled.LABEL_STYLE_REC_DTYPE.fields["text_position"][1]
    assert s(2) == C.sizeof(A.LabelBinding) == styled.LABEL_BINDING_DTYPE.itemsize == 8
    assert s(3) == C.sizeof(A.LabelBindingsDesc) and s(13) == A.LabelBindingsDesc.node_off.offset and s(14) == A.LabelBindingsDesc.n_chars.offset


def _refused(rc, code, *words):
    msg = lib.load().osmt_last_error().decode()
    assert rc == code and all(w in msg for w in words), (rc, msg)


def test_validators_without_a_context():
    L = lib.load()
    P = C.POINTER(A.LabelStyleRec)

    def styles(**kw):
        st = tl.label_styles([kw])
        return L.osmt_validate_label_styles(st.ctypes.data_as(P), 1, None)

    assert styles() == A.OK and styles(layer=3, z_index=-1.0, text_style=True) == A.OK
    _refused(styles(z_index=float("nan")), A.INVALID_ARG, "style 0", "NaN")
    _refused(styles(icon=0), A.INVALID_ARG, "icon_image 0", "not registered")  # a NULL context has no images
    _refused(styles(font_size=10.0), A.INVALID_ARG, "font_id 0", "not registered")  # and no fonts
    for bad in (float("inf"), float("nan"), 1e308):  # 1e308 * OSMT_MAX_SCALE is not finite
        _refused(styles(font_size=bad), A.INVALID_ARG, "font_size not finite")
    _refused(styles(text_position=3), A.INVALID_ARG, "text_position 3")
    assert L.osmt_validate_label_styles(None, 0, None) == A.OK
    _refused(L.osmt_validate_label_styles(None, 1, None), A.INVALID_ARG, "NULL")
    # a value whose has_* byte is 0 is not looked at
    st = tl.label_styles([{}])
    st["icon_image"], st["font_id"], st["font_size"] = 77, 99, float("nan")
    assert L.osmt_validate_label_styles(st.ctypes.data_as(P), 1, None) == A.OK
    # the tables that hang on a geodata id: a NULL context has none
    ix = styled.NodeIndex([1, 2], [[0, 1]])
    d = ix.as_desc()
    _refused(L.osmt_validate_node_index(C.byref(d), 0, None), A.INVALID_ARG, "geodata id 0", "no context")
    _refused(L.osmt_validate_node_index(None, 0, None), A.INVALID_ARG, "NULL")
    lb = styled.LabelBindings(0, 3, 9, [[(0, None)]], [])
    d = lb.as_desc()
    _refused(L.osmt_validate_label_bindings(C.byref(d), None), A.INVALID_ARG, "geodata id 0", "no context")
    for lo, hi in ((9, 3), (0, 19)):
        d = styled.LabelBindings(0, lo, hi, [[]], []).as_desc()
        _refused(L.osmt_validate_label_bindings(C.byref(d), None), A.INVALID_ARG, "zoom range")
    _refused(L.osmt_validate_label_bindings(None, None), A.INVALID_ARG, "NULL")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    r, refs, gids, nodes, bind = _world(tmp_path_factory.mktemp("tile_labels"))
    yield r, refs, gids, nodes, bind
    r.close()


def test_node_index_desc_reads_the_node_lists(world):
    r, refs, gids, _, _ = world
    h = tl.shim().tl_index_new(r.h)
    d = tl.shim().tl_index_get(h).contents
    want = tl.node_index_of(r, refs)
    assert d.n_nodes == len(gids) and [d.node_ids[i] for i in range(d.n_nodes)] == gids
    assert d.n_node_refs == len(want.nodes) and [d.node_off[i] for i in range(len(refs) + 1)] == want.node_off.tolist()
    assert [d.nodes[i] for i in range(d.n_node_refs)] == want.nodes.tolist()
    tl.shim().tl_index_free(h)


@pytest.mark.parametrize("scale", [1, 2, 3, 4])
def test_mirror_equals_the_restatement(world, scale):
    r, refs, gids, nodes, bind = world
    st = _styles()
    m = tl.Mirror(r, bind, TEXTS)
    seen = 0
    for zoom, x, y in TILES:
        pts = np.array([tl.py_project(la, lo, zoom, x, y, scale) for _, la, lo in nodes], dtype=np.int32)
        want = tl.restate(refs, gids, bind, TEXTS, st, ICON_H, zoom, x, y, scale, lambda n: pts[n])
        got = m.labels(st, ICON_H, zoom, x, y, scale, pts)
        for g, w, name in zip(got, want, ("labels", "runs", "chars")):
            assert g.shape == w.shape and np.array_equal(_u8(g), _u8(w)), (zoom, x, y, name)
        seen += len(want[0])
        if (zoom, x, y) == (18, CX, CY):  # the ties: node 0 and node 1 keep their push order among equal keys
            lab = got[0]
            of0 = [int(l["image_id"]) * 10 + int(l["has_text"]) for l in lab if l["icon_center_x"] == pts[0][0] and l["icon_center_y"] == pts[0][1]]
            assert of0 == [11, 1, 30], of0  # styles 2, 0, 1 in that order
        if zoom == 0:
            assert len(want[0]) == sum(len(b) for b in bind)  # the whole world, every node once
        # the libm projection of the mirror is the restatement's
        assert all(np.array_equal(_u8(a), _u8(b)) for a, b in zip(m.labels(st, ICON_H, zoom, x, y, scale), want))
    assert seen > 200
    assert m.labels(st, ICON_H, 18, CX + 100, CY, scale)[0].shape == (0,)
    m.close()


def test_libm_projection_equals_the_oracle(oracle):
    rng = np.random.default_rng(11)
    xy = (C.c_int32 * 2)()
    for zoom in (0, 7, 15, 18):
        n = 1 << zoom
        tx, ty = int(rng.integers(0, n)), int(rng.integers(0, n))
        ll = np.array([tl.latlon_of(zoom, tx + rng.uniform(-1.2, 2.2), ty + rng.uniform(-1.2, 2.2)) for _ in range(300)])
        ll[:, 0] = np.clip(ll[:, 0], -85.0, 85.0)
        ll[:, 1] = np.clip(ll[:, 1], -180.0, 180.0)
        for scale in (1.0, 2.0):
            want = oracle.project_points(ll, zoom, tx, ty, scale)
            for (la, lo), w in zip(ll, want):
                tl.shim().tl_project(la, lo, zoom, tx, ty, scale, xy)
                assert (xy[0], xy[1]) == tuple(w) == tl.py_project(la, lo, zoom, tx, ty, scale)


def test_mirror_under_sanitizers(world, tmp_path):
    """the fixed styles and binding rule of tests/tilelabels_host_main.cpp, restated here"""
    r, refs, gids, nodes, _ = world
    st = tl.label_styles([dict(font_size=11.5), dict(layer=0, z_index=-0.0, icon=3), dict(layer=-1, font_size=9.0, text_position=A.LABEL_POSITION_LINE),
                          dict(z_index=2.5, font_size=14.0, text_color=(200, 10, 30), text_position=A.LABEL_POSITION_CENTER)])
    icon_h = [0, 7, 0, 0]
    texts = ["ABC", ""]
    bind = [[((i + k) % 4, None if k % 2 else i % 2) for k in range(i % 4)] for i in range(len(nodes))]
    path = str(tmp_path / "w.bin")
    tl.write_geodata(path, [(g, la, lo, {}) for g, la, lo in nodes], [], [], [], tile_refs=refs)
    tiles = TILES[:7]
    out = subprocess.run([tl.build_host_main(), path, "2"] + [str(v) for t in tiles for v in t], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert lines[0] == f"index {len(nodes)} {len(refs)} {sum(len(v[0]) for v in refs.values())}"
    assert lines[1] == f"bindings {sum(len(b) for b in bind)} 2 3"
    k = 2
    for zoom, x, y in tiles:
        lab, runs, chars = tl.restate(refs, gids, bind, texts, st, icon_h, zoom, x, y, 2, lambda n: tl.py_project(nodes[n][1], nodes[n][2], zoom, x, y, 2))
        assert lines[k] == f"tile {zoom} {x} {y} {len(lab)} {len(chars)}"
        for l, s in zip(lab, runs):
            got = lines[k + 1].split()
            want = [l["has_icon"], l["has_text"], l["image_id"], l["seg_off"], l["n_segs"], s["y_offset"]]
            assert [int(v) for v in got[:6]] == [int(v) for v in want] and [int(v) for v in got[9:]] == l["text_color"].tolist()
            assert [float(v) for v in got[6:9]] == [float(s["font_size"]), float(l["icon_center_x"]), float(l["icon_center_y"])]
            k += 1
        k += 1
    assert k == len(lines)
