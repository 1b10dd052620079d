"""What the feed costs: host-built display lists against display lists built on the GPU, on the same tiles.

Workload: N z15 tiles (default 1024) over a synthetic world with config 2's per-tile content — 50 closed ways and 40 open
ways of 6 nodes per tile, every tile with ways of its own — written as a geodata file, and a table of 64 styles.

  (a) the host feed:   osmt::SceneBuilder::add_tile for every tile on one thread, then osmt_scene_upload
  (b) the device feed: osmt_scene_build_styled over the registered geodata and styles (8 bytes per styled area)

Both are timed in one process, alternating, from the caller's arrays to a scene that is complete on the device (each
library call synchronises its stream before it returns); then each scene is rendered once and the pixels are compared.
The device time of the new kernels comes from a child run with OSMT_TRACE_UPLOAD=1 (HIP events around the two launch
sequences).  PCIe bytes are computed from the shapes.  One JSON document on stdout and in profiles/styled_feed_bench.json.

    python tools/bench_styled_feed.py [--tiles 1024] [--reps 12] [--warmup 3] [--out profiles/styled_feed_bench.json]

--tiles-only runs another pair on the same world, written this time with its z18 tile index (every way in the z18 tiles its
nodes span) and with one style bound to every way:

  (c) the host query:  GeodataReader::get_entities_in_tile_with_neighbors + the style lookup per entity for every tile on one
                       thread (osmt::styled_areas_of_tile), then osmt_scene_build_styled
  (d) tiles only:      osmt_scene_build_tiles over the registered index and bindings (16 bytes per tile)

timed the same way — scene build only, and build + one render —, the stages of (d) from OSMT_TRACE_UPLOAD=1 in a child run.
Output: profiles/tile_query_bench.json.

--labels runs a third pair on a world of labelled nodes (24 per tile: text, icon + text, icon only), over one scene of
osmt_scene_build_tiles:

  (e) the host labels:   osmt::node_labels_of_tile for every tile on one thread (query, style lookup, stable sort,
                         Point::from_node, records), then osmt_scene_set_string_labels
  (f) the device labels: osmt_scene_build_tile_labels over the registered node index, label styles and label bindings

timed the same way, from the call to labels attached to the scene; the stages of (f) and the size of its read-back from
OSMT_TRACE_UPLOAD=1 in a child run.  Output: profiles/tile_labels_bench.json.

--area-labels runs a fourth pair on the world of (a) / (b), written with its z18 tile index, every closed way labelled with
an icon and a centred name, every open way with a name along the line, and five multipolygons per tile with a centred name:

  (g) the caller's way:  per tile the query, the style lookup and the pairs that need an anchor; one
                         osmt_label_positions_tiles; per tile osmt::area_labels_of_entities (order, Point::from_node, records, way
                         points, libm angles) on one thread (tools/area_labels_bench.cpp); then osmt_scene_build_tile_labels
                         with the batch as area_labels
  (h) the device labels: osmt_scene_build_tile_labels_all over the registered area label bindings

timed the same way, from the call to labels attached; the stages of (h), the share of its host angle loop and the size of its
read-back from OSMT_TRACE_UPLOAD=1 in a child run.  Output: profiles/area_labels_bench.json.
"""
import argparse
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from osm_renderer_amd import abi, lib, styled  # noqa: E402
from osm_renderer_amd.renderer import Context, Scene  # noqa: E402
from tests._geodata import write_geodata  # noqa: E402
from tests._styled_feed import recs_of  # noqa: E402
from tests.test_styled_builder import _random_styles  # noqa: E402

SO = os.path.join(ROOT, "tests", "_build", "libstyled_feed_bench.so")
ZOOM, X0, Y0 = 15, 19800, 10250


def _native():
    src = os.path.join(ROOT, "tools", "styled_feed_bench.cpp")
    deps = [src, os.path.join(ROOT, "tests", "styled_shim.cpp"), os.path.join(ROOT, "osm_renderer_amd", "host", "osmt_styled.hpp"), lib.LIB_PATH]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        pkg = os.path.join(ROOT, "osm_renderer_amd")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SO, src, "-L" + pkg, "-losmtile", "-Wl,-rpath," + pkg,
                               "-Wl,-rpath-link,/opt/rocm/lib"])
    lib.load()  # libosmtile.so (and the HIP runtime it binds to) first
    L = C.CDLL(SO)
    vp, sz = C.c_void_p, C.c_size_t
    L.sfb_new.restype = vp
    L.sfb_new.argtypes = [C.c_char_p, vp, sz, vp]
    L.sfb_free.argtypes = [vp]
    L.sfb_add_tile.argtypes = [vp, C.c_uint8, C.c_uint32, C.c_uint32, vp, vp, sz]
    L.sfb_run_host_feed.argtypes = [vp, vp, C.c_uint32, vp, C.POINTER(vp), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.sfb_run_device_feed.argtypes = [vp, C.POINTER(abi.StyledBatch), C.POINTER(vp), C.POINTER(C.c_double)]
    return L


def _latlon(px, py):
    """pixel coordinates at ZOOM (256 per tile) -> (lat, lon) degrees"""
    n = 256.0 * (1 << ZOOM)
    return math.degrees(math.atan(math.sinh(math.pi * (1.0 - 2.0 * py / n)))), px / n * 360.0 - 180.0


def make_world(n_tiles, seed=2):
    """config 2's content per tile: 50 closed ways (7-gons), 40 open ways of 6 nodes"""
    rng = np.random.default_rng(seed)
    side = int(math.ceil(math.sqrt(n_tiles)))
    nodes, ways, tiles = [], [], []
    for t in range(n_tiles):
        tx, ty = X0 + t % side, Y0 + t // side
        ids = []
        for k in range(90):
            cx, cy = rng.uniform(10, 246, 2)
            if k < 50:
                rad, ang = rng.uniform(4.0, 24.0), np.sort(rng.uniform(0, 2 * np.pi, 7))
                pts = [(cx + rad * math.cos(a), cy + rad * math.sin(a)) for a in ang]
                pts.append(pts[0])
            else:
                pts = [(cx, cy)]
                for _ in range(5):
                    pts.append((pts[-1][0] + rng.uniform(-20, 20), pts[-1][1] + rng.uniform(-20, 20)))
            first = len(nodes)
            for i, (x, y) in enumerate(pts[:-1] if k < 50 else pts):
                lat, lon = _latlon(256.0 * tx + x, 256.0 * ty + y)
                nodes.append((10**6 + len(nodes), lat, lon, {}))
            nid = list(range(first, len(nodes)))
            if k < 50:
                nid.append(first)
            ways.append((2 * 10**6 + len(ways), nid, {}))
            ids.append(len(ways) - 1)
        tiles.append((ZOOM, tx, ty, ids))
    return nodes, ways, tiles


def device_times(args):
    """the same workload in a child with OSMT_TRACE_UPLOAD=1: medians of the two launch sequences of osmt_scene_build_styled"""
    env = dict(os.environ, OSMT_TRACE_UPLOAD="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--tiles", str(args.tiles), "--reps", str(args.reps), "--warmup", str(args.warmup),
                        "--child"], env=env, capture_output=True, text=True, timeout=900)
    rows = re.findall(r"osmt styled build: sort \+ count \+ scan kernels ([0-9.]+) us, emit kernels ([0-9.]+) us", p.stderr)
    if p.returncode != 0 or len(rows) <= args.warmup:
        raise RuntimeError("the traced child run failed:\n" + p.stderr[-2000:])
    rows = np.array(rows[args.warmup:], dtype=np.float64)
    return {"count_us_median": float(np.median(rows[:, 0])), "emit_us_median": float(np.median(rows[:, 1])),
            "total_us_median": float(np.median(rows.sum(axis=1))), "runs": int(len(rows))}


def tiles_only(args):
    import time

    import torch

    from tests import _tilequery as tq
    from tests._geodata import Reader

    rng = np.random.default_rng(1)
    st, pool = _random_styles(rng, 64)
    nodes, ways, tiles = make_world(args.tiles)
    tmp = tempfile.mkdtemp(prefix="tile_query_")
    path = os.path.join(tmp, "world.bin")
    refs = write_geodata(path, nodes, ways, max_zoom_tile=tq.max_zoom_tile)
    r = Reader(path)
    ctx = Context(0)
    geo = styled.Geodata([[n[1], n[2]] for n in nodes], [(w[0], w[1]) for w in ways])
    gid = ctx.register_geodata(geo)
    first = ctx.register_styles(recs_of(st), pool)
    ctx.register_tile_index(gid, tq.index_of(refs))
    ws = [[int(s) + first] for s in rng.integers(0, len(st), len(ways))]
    bid = ctx.register_style_bindings(styled.StyleBindings(gid, 0, 18, ws, []))
    mir = tq.Mirror(r, ws, [], gid)
    zxy = np.array([(z, x, y) for z, x, y, _ in tiles], dtype=np.uint32)
    tb = styled.TileBatch(gid, [(z, x, y) for z, x, y, _ in tiles], {ZOOM: bid})
    S = tq.shim()
    sb = styled.StyledBatch(gid, [(z, x, y, [], []) for z, x, y, _ in tiles])
    cap = S.tq_batch(r.h, mir.h, zxy.ctypes.data, len(zxy), sb.tiles.ctypes.data, None, 0)
    sb.areas = np.zeros(cap, styled.STYLED_AREA_DTYPE)

    def run(which, render):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if which == "c":
            n = S.tq_batch(r.h, mir.h, zxy.ctypes.data, len(zxy), sb.tiles.ctypes.data, sb.areas.ctypes.data, cap)
            assert n == cap
            t1 = time.perf_counter()
            scene = ctx.build_styled(sb)
        else:
            t1 = t0
            scene = ctx.build_tiles(tb)
        t2 = time.perf_counter()
        if render:
            ctx.render(scene)
            torch.cuda.synchronize()
        t3 = time.perf_counter()
        return scene, (t1 - t0, t2 - t0, t3 - t0)

    times = {(w, rd): [] for w in "cd" for rd in (False, True)}
    for rep in range(args.warmup + args.reps):
        for render in (False, True):
            for which in ("c", "d") if rep % 2 == 0 else ("d", "c"):
                scene, t = run(which, render)
                scene.free()
                if rep >= args.warmup:
                    times[(which, render)].append(t)
    if args.child:
        return
    sc, _ = run("c", False)
    sd, _ = run("d", False)
    dl_c, dl_d = sc.read_display_list(), sd.read_display_list()
    same_list = all(getattr(dl_c, k).tobytes() == getattr(dl_d, k).tobytes() for k in ("jobs", "ops", "rings", "coords", "dashes"))
    t_d, a_d = sd.read_styled_areas()
    same_areas = bool(a_d.tobytes() == sb.areas.tobytes() and np.array_equal(t_d["n_areas"], sb.tiles["n_areas"]))
    same_px = bool(np.array_equal(ctx.render(sc).cpu().numpy(), ctx.render(sd).cpu().numpy()))
    n_ops = len(dl_d.ops)
    sc.free()
    sd.free()

    def stat(rows, k):
        v = np.array([row[k] for row in rows])
        return {"median_ms": float(np.median(v) * 1e3), "min_ms": float(v.min() * 1e3), "max_ms": float(v.max() * 1e3),
                "p25_ms": float(np.percentile(v, 25) * 1e3), "p75_ms": float(np.percentile(v, 75) * 1e3), "runs": len(v)}

    env = dict(os.environ, OSMT_TRACE_UPLOAD="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--tiles-only", "--tiles", str(args.tiles), "--reps", str(args.reps), "--warmup",
                        str(args.warmup), "--child"], env=env, capture_output=True, text=True, timeout=900)
    names = ("span", "columns", "gather", "sort", "mark_scan", "emit")
    rows = re.findall(r"osmt tile query: span ([0-9.]+) us, columns ([0-9.]+) us, gather ([0-9.]+) us, sort ([0-9.]+) us, mark \+ scan ([0-9.]+) us, "
                      r"emit ([0-9.]+) us", p.stderr)
    if p.returncode != 0 or len(rows) <= 2 * args.warmup:
        raise RuntimeError("the traced child run failed:\n" + p.stderr[-2000:])
    rows = np.array(rows[2 * args.warmup:], dtype=np.float64)
    T, A = len(tiles), int(cap)
    res = {
        "workload": {"tiles": T, "zoom": ZOOM, "ways": len(ways), "index_tiles": len(refs), "way_refs_in_index": int(sum(len(v[1]) for v in refs.values())),
                     "styles": int(len(st)), "areas": A, "ops": n_ops},
        "host_query_c": {"query_and_lookup": stat(times[("c", False)], 0), "scene_build": stat(times[("c", False)], 1),
                         "build_and_render": stat(times[("c", True)], 2)},
        "tiles_only_d": {"scene_build": stat(times[("d", False)], 1), "build_and_render": stat(times[("d", True)], 2)},
        "host_ms_removed_median": float(np.median([t[0] for t in times[("c", False)]]) * 1e3),
        "build_speedup_median_c_over_d": float(np.median([t[1] for t in times[("c", False)]]) / np.median([t[1] for t in times[("d", False)]])),
        "device_stages_d_us_median": dict({n: float(np.median(rows[:, i])) for i, n in enumerate(names)}, total=float(np.median(rows.sum(axis=1))),
                                          runs=int(len(rows))),
        "bytes_sent_per_tile": {"host_query_c": (24 * T + 4 * (T + 1) + 8 * A) / T, "tiles_only_d": (16 * T + 32 * (abi.MAX_ZOOM + 1)) / T},
        "same_styled_areas": same_areas,
        "same_display_list": bool(same_list),
        "same_pixels": same_px,
    }
    text = json.dumps(res, indent=1)
    print(text)
    out = os.path.join(os.path.dirname(args.out), "tile_query_bench.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")
    if not (same_areas and same_list and same_px):
        sys.exit("the two feeds disagree")


def tile_labels(args):
    import time

    import torch

    from osm_renderer_amd import labels
    from tests import _tilelabels as tl
    from tests import _tilequery as tq
    from tests._geodata import Reader

    rng = np.random.default_rng(3)
    side = int(math.ceil(math.sqrt(args.tiles)))
    tiles = [(ZOOM, X0 + t % side, Y0 + t // side) for t in range(args.tiles)]
    per_tile = 24
    nodes = []
    for _, tx, ty in tiles:
        for _ in range(per_tile):
            x, y = rng.uniform(6, 250, 2)
            lat, lon = _latlon(256.0 * tx + x, 256.0 * ty + y)
            nodes.append((10**6 + len(nodes), lat, lon, {}))
    tmp = tempfile.mkdtemp(prefix="tile_labels_")
    path = os.path.join(tmp, "world.bin")
    refs = write_geodata(path, nodes, max_zoom_tile=tq.max_zoom_tile)
    r = Reader(path)
    ctx = Context(0)
    syn = labels.synth_glyph_table()
    ctx.register_glyphs(syn)
    ns = len(labels.SYNTH_GLYPHS)
    shapes = [ns - 1] + [(g - 1) % (ns - 1) for g in range(1, 13)] + [ns - 1]
    font = labels.FontTable([(0x20, 13)] + [(0x41 + i, 1 + i) for i in range(12)], [300] + [labels.SYNTH_GLYPHS[s][0] for s in shapes[1:]],
                            [syn.first_id + s for s in shapes])
    ctx.register_font(font)
    icon = ctx.register_image(rng.integers(0, 256, size=(12, 12, 4)).astype(np.uint8))
    gid = ctx.register_geodata(styled.Geodata([[n[1], n[2]] for n in nodes]))
    ctx.register_tile_index(gid, styled.TileIndex([(k, [], []) for k in sorted(refs)]))
    ctx.register_node_index(gid, styled.NodeIndex([n[0] for n in nodes], [sorted(refs[k][0]) for k in sorted(refs)]))
    area_bind = ctx.register_style_bindings(styled.StyleBindings(gid, 0, 18, [], []))
    rows = [dict(font_size=10.0, font_id=font.font_id), dict(layer=1, icon=icon, font_size=9.0, font_id=font.font_id, text_color=(120, 0, 40)),
            dict(z_index=2.0, icon=icon), dict(layer=-1, font_size=12.0, font_id=font.font_id, text_color=(0, 60, 160))]
    rec = tl.label_styles(rows)
    first = ctx.register_label_styles(rec)
    all_styles = np.concatenate([np.zeros(first, styled.LABEL_STYLE_REC_DTYPE), rec])
    icon_h = np.array([0] * first + [0, 12, 12, 0], dtype=np.uint32)
    texts = ["".join(chr(0x41 + int(c)) for c in rng.integers(0, 12, int(n))) for n in rng.integers(4, 13, 64)]
    bind = [[(first + int(rng.integers(0, 4)), int(rng.integers(0, len(texts))))] for _ in nodes]
    lbid = ctx.register_label_bindings(styled.LabelBindings(gid, 0, 18, bind, texts))
    mir = tl.Mirror(r, bind, texts, gid)
    scene = ctx.build_tiles(styled.TileBatch(gid, tiles, {ZOOM: area_bind}))
    zxy = np.array(tiles, dtype=np.uint32)
    S, L = tl.shim(), lib.load()
    sz2 = C.c_size_t * 2
    caps, n = sz2(per_tile * 9 * len(tiles), per_tile * 9 * len(tiles) * 12), sz2()
    lab, runs = np.zeros(caps[0], labels.LABEL_DTYPE), np.zeros(caps[0], labels.STRING_RUN_DTYPE)
    chars, off = np.zeros(caps[1], np.uint32), np.zeros(len(tiles) + 1, np.uint32)
    ids = (C.c_uint32 * (abi.MAX_ZOOM + 1))(*[lbid if z == ZOOM else abi.BINDINGS_NONE for z in range(abi.MAX_ZOOM + 1)])

    def host_batch():
        S.tl_batch(r.h, mir.h, all_styles.ctypes.data, icon_h.ctypes.data_as(C.POINTER(C.c_uint32)), len(all_styles), zxy.ctypes.data, len(zxy), 1,
                   lab.ctypes.data, runs.ctypes.data, chars.ctypes.data, off.ctypes.data, caps, n)
        assert n[0] <= caps[0] and n[1] <= caps[1]
        return labels.StringLabelList(lab[: n[0]], off, runs[: n[0]], chars[: n[1]], np.zeros((0, 2), np.int32), np.zeros((0, 2)))

    def run(which, render):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if which == "e":
            sl = host_batch()
            t1 = time.perf_counter()
            sb = sl.as_batch()
            lib.check(L.osmt_scene_set_string_labels(ctx._h, scene._h, C.byref(sb)))
        else:
            t1 = t0
            lib.check(L.osmt_scene_build_tile_labels(ctx._h, scene._h, ids, None))
        t2 = time.perf_counter()
        if render:
            ctx.render(scene)
            torch.cuda.synchronize()
        return t1 - t0, t2 - t0, time.perf_counter() - t0

    times = {(w, rd): [] for w in "ef" for rd in (False, True)}
    for rep in range(args.warmup + args.reps):
        for render in (False, True):
            for which in ("e", "f") if rep % 2 == 0 else ("f", "e"):
                t = run(which, render)
                if rep >= args.warmup:
                    times[(which, render)].append(t)
    if args.child:
        return
    run("e", False)
    want = host_batch()
    px_e = ctx.render(scene).cpu().numpy()
    st_e = np.zeros(len(want.labels), np.uint8)
    lib.check(L.osmt_scene_read_label_status(ctx._h, scene._h, st_e.ctypes.data_as(C.POINTER(C.c_uint8))))
    run("f", False)
    got = scene.read_tile_labels()
    same_batch = bool(all(getattr(got, k).tobytes() == getattr(want, k).tobytes() for k in ("labels", "runs", "chars", "job_label_off")))
    px_f = ctx.render(scene).cpu().numpy()
    st_f = np.zeros(len(got.labels), np.uint8)
    lib.check(L.osmt_scene_read_label_status(ctx._h, scene._h, st_f.ctypes.data_as(C.POINTER(C.c_uint8))))
    same_px = bool(np.array_equal(px_e, px_f) and np.array_equal(st_e, st_f))

    def stat(rows, k):
        v = np.array([row[k] for row in rows])
        return {"median_ms": float(np.median(v) * 1e3), "min_ms": float(v.min() * 1e3), "max_ms": float(v.max() * 1e3),
                "p25_ms": float(np.percentile(v, 25) * 1e3), "p75_ms": float(np.percentile(v, 75) * 1e3), "runs": len(v)}

    env = dict(os.environ, OSMT_TRACE_UPLOAD="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--labels", "--tiles", str(args.tiles), "--reps", str(args.reps), "--warmup",
                        str(args.warmup), "--child"], env=env, capture_output=True, text=True, timeout=900)
    names = ("span_columns", "gather_sort", "mark_scan", "expand_sort_count", "emit")
    rows = re.findall(r"osmt tile labels: span \+ columns ([0-9.]+) us, gather \+ sort ([0-9.]+) us, mark \+ scan ([0-9.]+) us, expand \+ sort \+ count "
                      r"([0-9.]+) us, emit ([0-9.]+) us .*?, (\d+) bytes read back", p.stderr)
    if p.returncode != 0 or len(rows) <= 2 * args.warmup:
        raise RuntimeError("the traced child run failed:\n" + p.stderr[-2000:])
    rows = np.array(rows[2 * args.warmup:], dtype=np.float64)
    med = lambda w, rd, k: float(np.median([t[k] for t in times[(w, rd)]]))
    res = {
        "workload": {"tiles": len(tiles), "zoom": ZOOM, "nodes": len(nodes), "index_tiles": len(refs), "label_styles": int(len(rec)),
                     "labels": int(len(want.labels)), "chars": int(len(want.chars)), "labels_placed": int(st_f.sum())},
        "host_labels_e": {"mirror": stat(times[("e", False)], 0), "labels_attached": stat(times[("e", False)], 1),
                          "attach_and_render": stat(times[("e", True)], 2)},
        "device_labels_f": {"labels_attached": stat(times[("f", False)], 1), "attach_and_render": stat(times[("f", True)], 2)},
        "speedup_median_e_over_f": med("e", False, 1) / med("f", False, 1),
        "device_path_is_faster": bool(med("f", False, 1) < med("e", False, 1)),
        "device_stages_f_us_median": dict({k: float(np.median(rows[:, i])) for i, k in enumerate(names)}, total=float(np.median(rows[:, :5].sum(axis=1))),
                                          runs=int(len(rows))),
        "read_back_bytes_f": int(rows[-1, 5]),
        "bytes_sent": {"host_labels_e": int(want.input_bytes()), "device_labels_f": int(want.input_bytes()),
                       "note": "(f) reads the batch back and hands it to the string-label path, which uploads it again"},
        "same_batch": same_batch,
        "same_pixels_and_statuses": same_px,
    }
    text = json.dumps(res, indent=1)
    print(text)
    out = os.path.join(os.path.dirname(args.out), "tile_labels_bench.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")
    if not same_px:
        sys.exit("the two label feeds disagree")


def area_labels(args):
    import time

    import torch

    from osm_renderer_amd import labels
    from tests import _anchors as an
    from tests import _tilelabels as tl
    from tests import _tilequery as tq

    rng = np.random.default_rng(7)
    nodes, ways, tiles = make_world(args.tiles)
    polygons, mps = [], []
    for t, (_, _, _, ids) in enumerate(tiles):  # five multipolygons per tile over the outlines of its first closed ways
        for k in range(5):
            polygons.append(list(ways[ids[k]][1]))
            mps.append((5 * 10**6 + len(mps), [len(polygons) - 1], {}))
    tmp = tempfile.mkdtemp(prefix="area_labels_")
    path = os.path.join(tmp, "world.bin")
    refs = write_geodata(path, nodes, ways, polygons, mps, max_zoom_tile=tq.max_zoom_tile)
    ctx = Context(0)
    syn = labels.synth_glyph_table()
    ctx.register_glyphs(syn)
    ns = len(labels.SYNTH_GLYPHS)
    shapes = [ns - 1] + [(g - 1) % (ns - 1) for g in range(1, 13)] + [ns - 1]
    font = labels.FontTable([(0x20, 13)] + [(0x41 + i, 1 + i) for i in range(12)], [300] + [labels.SYNTH_GLYPHS[s][0] for s in shapes[1:]],
                            [syn.first_id + s for s in shapes])
    ctx.register_font(font)
    icon = ctx.register_image(rng.integers(0, 256, size=(12, 12, 4)).astype(np.uint8))
    geo = styled.Geodata([[n[1], n[2]] for n in nodes], [(w[0], w[1]) for w in ways], polygons, [(m[0], m[1]) for m in mps])
    gid = ctx.register_geodata(geo)
    keys = sorted(refs)
    ctx.register_tile_index(gid, styled.TileIndex([(k, sorted(refs[k][1]), sorted(refs[k][2])) for k in keys]))
    ctx.register_node_mercator(gid, an.mercator_factors(geo.nodes))
    ctx.register_node_index(gid, styled.NodeIndex([n[0] for n in nodes], [[] for _ in keys]))
    draw_bind = ctx.register_style_bindings(styled.StyleBindings(gid, 0, 18, [[] for _ in ways], [[] for _ in mps]))
    rows = [dict(layer=1, icon=icon, font_size=9.0, font_id=font.font_id, text_color=(120, 0, 40), text_position=abi.LABEL_POSITION_CENTER),
            dict(font_size=10.0, font_id=font.font_id), dict(z_index=2.0, font_size=11.0, font_id=font.font_id, text_color=(0, 60, 160))]
    rec = tl.label_styles(rows)
    first = ctx.register_label_styles(rec)
    all_styles = np.concatenate([np.zeros(first, styled.LABEL_STYLE_REC_DTYPE), rec])
    icon_h = np.array([0] * first + [12, 0, 0], dtype=np.uint32)
    texts = ["".join(chr(0x41 + int(c)) for c in rng.integers(0, 12, int(n))) for n in rng.integers(4, 13, 64)]
    closed = [len(w[1]) >= 2 and w[1][0] == w[1][-1] for w in ways]
    wb = [[(first + (0 if c else 1), int(rng.integers(0, len(texts))))] for c in closed]
    mb = [[(first + 2, int(rng.integers(0, len(texts))))] for _ in mps]
    tab = styled.AreaLabelBindings(gid, 0, 18, wb, mb, texts)
    abid = ctx.register_area_label_bindings(tab)
    nbid = ctx.register_label_bindings(styled.LabelBindings(gid, 0, 18, [[] for _ in nodes], []))
    qt = [(z, x, y) for z, x, y, _ in tiles]
    scene = ctx.build_tiles(styled.TileBatch(gid, qt, {ZOOM: draw_bind}))
    L = lib.load()
    so = os.path.join(ROOT, "tests", "_build", "libarea_labels_bench.so")
    src = os.path.join(ROOT, "tools", "area_labels_bench.cpp")
    hdr = os.path.join(ROOT, "osm_renderer_amd", "host", "osmt_arealabels.hpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in (src, hdr, lib.LIB_PATH)):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        pkg = os.path.join(ROOT, "osm_renderer_amd")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src, "-L" + pkg, "-losmtile", "-Wl,-rpath," + pkg,
                               "-Wl,-rpath-link,/opt/rocm/lib"])
    N = C.CDLL(so)
    vp, sz, u32p = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)
    N.alb_new.restype = vp
    N.alb_new.argtypes = [C.c_char_p, C.c_uint32, u32p, vp, u32p, vp, sz, u32p, u32p, vp, u32p, sz]
    N.alb_run.argtypes = [vp, vp, C.c_uint32, vp, sz, C.c_uint32, C.POINTER(C.c_double), C.POINTER(sz)]
    N.alb_batch.argtypes = [vp, C.POINTER(abi.StringLabelBatch)]
    N.alb_free.argtypes = [vp]
    h = N.alb_new(path.encode(), gid, tab.way_off.ctypes.data_as(u32p), tab.way_bindings.ctypes.data, tab.multipolygon_off.ctypes.data_as(u32p),
                  tab.multipolygon_bindings.ctypes.data, len(tab.text_off) - 1, tab.text_off.ctypes.data_as(u32p), tab.chars.ctypes.data_as(u32p),
                  all_styles.ctypes.data, icon_h.ctypes.data_as(u32p), len(all_styles))
    assert h
    qtiles = np.zeros(len(qt), styled.QUERY_TILE_DTYPE)
    qtiles["zoom"], qtiles["x"], qtiles["y"] = [t[0] for t in qt], [t[1] for t in qt], [t[2] for t in qt]
    a_ids = (C.c_uint32 * (abi.MAX_ZOOM + 1))(*[abid if z == ZOOM else abi.BINDINGS_NONE for z in range(abi.MAX_ZOOM + 1)])
    n_ids = (C.c_uint32 * (abi.MAX_ZOOM + 1))(*[nbid if z == ZOOM else abi.BINDINGS_NONE for z in range(abi.MAX_ZOOM + 1)])
    sec, cnt = (C.c_double * 3)(), (sz * 4)()

    def run(which):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if which == "g":
            lib.check(N.alb_run(h, ctx._h, gid, qtiles.ctypes.data, len(qtiles), 1, sec, cnt))
            sb = abi.StringLabelBatch()
            N.alb_batch(h, C.byref(sb))
            t1 = time.perf_counter()
            lib.check(L.osmt_scene_build_tile_labels(ctx._h, scene._h, n_ids, C.byref(sb)))
            return (sec[0], sec[1], sec[2], t1 - t0, time.perf_counter() - t0)
        lib.check(L.osmt_scene_build_tile_labels_all(ctx._h, scene._h, a_ids, n_ids, None, 0))
        return (0.0, 0.0, 0.0, 0.0, time.perf_counter() - t0)

    times = {"g": [], "h": []}
    for rep in range(args.warmup + args.reps):
        for which in ("g", "h") if rep % 2 == 0 else ("h", "g"):
            t = run(which)
            if rep >= args.warmup:
                times[which].append(t)
    if args.child:
        return

    def look(n_labels):
        px = ctx.render(scene).cpu().numpy()
        st = np.zeros(n_labels, np.uint8)
        lib.check(L.osmt_scene_read_label_status(ctx._h, scene._h, st.ctypes.data_as(C.POINTER(C.c_uint8))))
        return px, st

    run("g")
    counts_g = [int(v) for v in cnt]
    px_g, st_g = look(counts_g[0])
    run("h")
    got = scene.read_tile_area_labels()
    px_h, st_h = look(len(got.labels))
    same_px = bool(np.array_equal(px_g, px_h) and np.array_equal(st_g, st_h))
    same_counts = counts_g[:3] == [len(got.labels), len(got.chars), len(got.way_pts)]

    def stat(rows, k):
        v = np.array([row[k] for row in rows])
        return {"median_ms": float(np.median(v) * 1e3), "min_ms": float(v.min() * 1e3), "max_ms": float(v.max() * 1e3),
                "p25_ms": float(np.percentile(v, 25) * 1e3), "p75_ms": float(np.percentile(v, 75) * 1e3), "runs": len(v)}

    env = dict(os.environ, OSMT_TRACE_UPLOAD="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--area-labels", "--tiles", str(args.tiles), "--reps", str(args.reps), "--warmup",
                        str(args.warmup), "--child"], env=env, capture_output=True, text=True, timeout=900)
    names = ("query", "expand_sort", "anchors", "count_scans", "emit", "host_angles")
    rows = re.findall(r"osmt area labels: query ([0-9.]+) us, expand \+ sort ([0-9.]+) us, anchors ([0-9.]+) us, count \+ scans ([0-9.]+) us, emit ([0-9.]+) us, "
                      r"host angles ([0-9.]+) us .*?, (\d+) anchor requests, .*?, (\d+) bytes read back", p.stderr)
    if p.returncode != 0 or len(rows) <= args.warmup:
        raise RuntimeError("the traced child run failed:\n" + p.stderr[-2000:])
    rows = np.array(rows[args.warmup:], dtype=np.float64)
    g_all, h_all = np.array([t[4] for t in times["g"]]), np.array([t[4] for t in times["h"]])
    kernels_us = float(np.median(rows[:, :5].sum(axis=1)))
    res = {
        "workload": {"tiles": len(qt), "zoom": ZOOM, "ways": len(ways), "multipolygons": len(mps), "index_tiles": len(keys), "labels": len(got.labels),
                     "chars": len(got.chars), "way_points": len(got.way_pts), "anchor_requests": int(rows[-1, 6]), "labels_placed": int(st_h.sum())},
        "caller_g": {"query_and_requests": stat(times["g"], 0), "osmt_label_positions_tiles": stat(times["g"], 1), "records": stat(times["g"], 2),
                     "batch_built": stat(times["g"], 3), "labels_attached": stat(times["g"], 4)},
        "device_h": {"labels_attached": stat(times["h"], 4)},
        "speedup_median_g_over_h": float(np.median(g_all) / np.median(h_all)),
        "device_path_is_faster": bool(h_all.max() < g_all.min()),
        "caller_path_is_faster": bool(g_all.max() < h_all.min()),
        "device_stages_h_us_median": dict({k: float(np.median(rows[:, i])) for i, k in enumerate(names)}, kernels_total=kernels_us, runs=int(len(rows))),
        "share_of_h": {"new_kernels_and_query": kernels_us * 1e-6 / float(np.median(h_all)), "host_angle_loop": float(np.median(rows[:, 5])) * 1e-6 / float(np.median(h_all))},
        "read_back_bytes_h": int(rows[-1, 7]),
        "same_label_chars_and_way_point_counts": bool(same_counts),
        "same_pixels_and_statuses": same_px,
        "note": "(g) projects with the host's libm, (h) on the device: a rounding tie may move a way point by one; pixels and statuses are compared",
    }
    text = json.dumps(res, indent=1)
    print(text)
    out = os.path.join(os.path.dirname(args.out), "area_labels_bench.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")
    N.alb_free(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "styled_feed_bench.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tiles-only", action="store_true", help="the tile-query pair (c) / (d) instead of (a) / (b)")
    ap.add_argument("--labels", action="store_true", help="the node-label pair (e) / (f) instead of (a) / (b)")
    ap.add_argument("--area-labels", action="store_true", help="the area-label pair (g) / (h) instead of (a) / (b)")
    args = ap.parse_args()
    assert args.reps >= 10 or args.child
    if args.tiles_only:
        return tiles_only(args)
    if args.labels:
        return tile_labels(args)
    if args.area_labels:
        return area_labels(args)

    L = _native()
    rng = np.random.default_rng(1)
    st, pool = _random_styles(rng, 64)
    nodes, ways, tiles = make_world(args.tiles)
    way_style = [rng.integers(0, len(st), len(ids)).astype(np.uint32) for _, _, _, ids in tiles]
    tmp = tempfile.mkdtemp(prefix="styled_feed_")
    path = os.path.join(tmp, "world.bin")
    write_geodata(path, nodes, ways, tile_refs={})
    ctx = Context(0)
    geo = styled.Geodata([[n[1], n[2]] for n in nodes], [(w[0], w[1]) for w in ways])
    gid = ctx.register_geodata(geo)
    first = ctx.register_styles(recs_of(st), pool)
    h = L.sfb_new(path.encode(), st.ctypes.data, len(st), pool.ctypes.data)
    assert h
    for (zoom, tx, ty, ids), ws in zip(tiles, way_style):
        wi = np.array(ids, dtype=np.uint32)
        L.sfb_add_tile(h, zoom, tx, ty, wi.ctypes.data, ws.ctypes.data, len(wi))
    sb = styled.StyledBatch(gid, [(z, x, y, [(i, int(s) + first) for i, s in zip(ids, ws)], []) for (z, x, y, ids), ws in zip(tiles, way_style)])
    b = sb.as_batch()
    canvas = (C.c_uint8 * 3)(241, 238, 232)
    counts = (C.c_uint64 * 5)()

    def run(which):
        sc, sec = C.c_void_p(), C.c_double()
        if which == "a":
            rc = L.sfb_run_host_feed(h, ctx._h, 1, canvas, C.byref(sc), C.byref(sec), counts)
        else:
            rc = L.sfb_run_device_feed(ctx._h, C.byref(b), C.byref(sc), C.byref(sec))
        lib.check(rc)
        return sc, sec.value

    times = {"a": [], "b": []}
    for rep in range(args.warmup + args.reps):
        for which in ("a", "b") if rep % 2 == 0 else ("b", "a"):
            sc, sec = run(which)
            lib.load().osmt_scene_free(sc)
            if rep >= args.warmup:
                times[which].append(sec)
    if args.child:
        return
    # the pixels agree
    sa, _ = run("a")
    sb_, _ = run("b")
    scene_a, scene_b = Scene._built(ctx, sa, len(tiles), 1, geo.nodes), Scene._built(ctx, sb_, len(tiles), 1, geo.nodes)
    pa, pb = ctx.render(scene_a).cpu().numpy(), ctx.render(scene_b).cpu().numpy()
    scene_a.check()
    scene_b.check()
    same = bool(np.array_equal(pa, pb))
    dl_a, dl_b = scene_a.read_display_list(), scene_b.read_display_list()
    same_list = all(getattr(dl_a, k).tobytes() == getattr(dl_b, k).tobytes() for k in ("jobs", "ops", "rings", "coords", "dashes"))
    scene_a.free()
    scene_b.free()
    L.sfb_free(h)

    n_ops, n_rings, n_refs, n_dashes, n_nodes = (int(v) for v in counts)
    T, A = len(tiles), len(sb.areas)
    stat = lambda v: {"median_ms": float(np.median(v) * 1e3), "min_ms": float(np.min(v) * 1e3), "max_ms": float(np.max(v) * 1e3),
                      "p25_ms": float(np.percentile(v, 25) * 1e3), "p75_ms": float(np.percentile(v, 75) * 1e3), "runs": len(v)}
    res = {
        "workload": {"tiles": T, "zoom": ZOOM, "closed_ways_per_tile": 50, "open_ways_per_tile": 40, "styles": int(len(st)), "areas": A, "ops": n_ops,
                     "rings": n_rings, "node_refs": n_refs, "dashes": n_dashes, "nodes": n_nodes},
        "host_feed_a": stat(times["a"]),
        "device_feed_b": stat(times["b"]),
        "speedup_median_a_over_b": float(np.median(times["a"]) / np.median(times["b"])),
        "device_kernels_b": device_times(args),
        "pcie_bytes_per_batch": {
            # osmt_scene_upload: jobs, ops, rings, node refs, dashes, the node table, and the four op index tables
            "host_feed_a": 32 * T + 64 * n_ops + 8 * n_rings + 4 * n_refs + 8 * n_dashes + 16 * n_nodes + 16 * n_ops,
            # osmt_scene_build_styled: tiles, their area bases, areas; 64 bytes of totals back
            "device_feed_b": 24 * T + 4 * (T + 1) + 8 * A + 64,
            "registered_once_b": 16 * n_nodes + 8 * len(ways) + 4 * (len(ways) + 1) + 4 * len(geo.way_nodes) + 96 * len(st) + 4 * len(st) + 8 * len(pool),
        },
        "same_pixels": same,
        "same_display_list": bool(same_list),
    }
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    if not (same and same_list):
        sys.exit("the two feeds disagree")


if __name__ == "__main__":
    main()
