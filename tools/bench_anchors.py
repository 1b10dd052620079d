"""What the label anchors of tile-built scenes cost: host projection + osmt_label_positions against osmt_label_positions_tiles.

Workload: the areas of the 1024-tile z15 batch of tools/bench_styled_feed.py (50 closed 7-gons per tile).  A tile sees the areas
of its 3 x 3 neighbourhood, so every tile asks for the anchors of its own closed ways and of its neighbours' — about nine
requests per area.

  (g) the host path:   every node of every (tile, area) pair projected with libm on one thread (tan and log per node and per
                       pair, then the three operations of nodes_to_points), rings and points assembled, osmt_label_positions
  (h) the device path: osmt_label_positions_tiles over Mercator factors registered once per geodata file (16 B per node,
                       reported separately: it is paid once, not per batch)

Both are timed in one process, alternating, from the caller's arrays to the positions in host memory, and their positions are
compared bit for bit.  PCIe bytes are computed from the shapes.  Kernel times are not taken here: run the tool under a kernel
trace for a few repetitions and hand the kernel statistics to --kernel-stats, which copies the rows of the kernels involved
into the document.  One JSON document on stdout and in profiles/anchors_bench.json.

    python tools/bench_anchors.py [--tiles 1024] [--reps 12] [--warmup 3] [--scale 1] [--kernel-stats stats.csv [--merge-only]]
"""
import argparse
import csv
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from osm_renderer_amd import abi, labels, lib, styled  # noqa: E402
from osm_renderer_amd.renderer import Context  # noqa: E402

SO = os.path.join(ROOT, "tests", "_build", "libanchors_bench.so")
KERNELS = ("k_an_count", "k_an_rings", "k_an_records", "k_an_points", "k_tq_scan_local", "k_tq_scan_blocks", "k_tq_scan_apply", "k_polylabel",
           "k_polylabel_big")


def _native():
    src = os.path.join(ROOT, "tools", "anchors_bench.cpp")
    deps = [src, os.path.join(ROOT, "include", "osmtile.h"), lib.LIB_PATH]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        pkg = os.path.join(ROOT, "osm_renderer_amd")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", SO, src, "-L" + pkg, "-losmtile",
                               "-Wl,-rpath," + pkg, "-Wl,-rpath-link,/opt/rocm/lib"])
    lib.load()  # libosmtile.so (and the HIP runtime it binds to) first
    L = C.CDLL(SO)
    vp = C.c_void_p
    L.ab_host.argtypes = [vp, C.POINTER(abi.GeodataDesc), vp, vp, C.c_size_t, C.c_uint32, vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.ab_device.argtypes = [vp, C.POINTER(abi.LabelTileBatch), vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    return L


def workload(n_tiles):
    """(styled.Geodata, tiles as QUERY_TILE_DTYPE, requests as LABEL_TILE_REQUEST_DTYPE): every tile asks for the closed ways of
    its 3 x 3 neighbourhood"""
    from bench_styled_feed import make_world

    nodes, ways, tiles = make_world(n_tiles)
    g = styled.Geodata(np.array([(la, lo) for _, la, lo, _ in nodes]), [(gid, nid) for gid, nid, _ in ways])
    closed = {(x, y): [w for w in ids if ways[w][1][0] == ways[w][1][-1]] for _, x, y, ids in tiles}
    qt = np.zeros(len(tiles), styled.QUERY_TILE_DTYPE)
    reqs = []
    for t, (zoom, x, y, _) in enumerate(tiles):
        qt[t]["zoom"], qt[t]["x"], qt[t]["y"] = zoom, x, y
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                reqs += [(w, t) for w in closed.get((x + dx, y + dy), ())]
    return g, qt, np.array(reqs, dtype=labels.LABEL_TILE_REQUEST_DTYPE)


def kernel_rows(path):
    """the rows of a kernel statistics CSV (columns Name, Calls, TotalDurationNs, AverageNs, ...) that belong to the two paths"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for k in KERNELS:
                if k + "(" in name or name.endswith(k) or ("::" + k + "(") in name:
                    out[k] = {"calls": int(row["Calls"]), "total_us": float(row["TotalDurationNs"]) / 1e3, "average_us": float(row["AverageNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--kernel-stats", default=None, help="kernel statistics CSV of a traced run of this tool")
    ap.add_argument("--merge-only", action="store_true", help="no run: add --kernel-stats to the document --out already holds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anchors_bench.json"))
    args = ap.parse_args()
    if args.merge_only:
        with open(args.out) as fh:
            doc = json.load(fh)
        doc["kernels"] = kernel_rows(args.kernel_stats)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")
        return 0

    import time

    from tests import _anchors

    L = _native()
    g, qt, rq = workload(args.tiles)
    ctx = Context(0)
    gid = ctx.register_geodata(g)
    t0 = time.perf_counter()
    f = _anchors.mercator_factors(g.nodes)
    t_factors = time.perf_counter() - t0
    t0 = time.perf_counter()
    ctx.register_node_mercator(gid, f)
    t_register = time.perf_counter() - t0
    d = g.as_desc()
    b, _keep = ctx._label_tile_batch(gid, qt, rq, args.scale)
    out_h, out_d = np.zeros(len(rq), labels.LABEL_POSITION_DTYPE), np.zeros(len(rq), labels.LABEL_POSITION_DTYPE)
    ms2, ms1, by_h, by_d = (C.c_double * 2)(), C.c_double(), C.c_uint64(), C.c_uint64()
    host, dev = [], []
    for rep in range(args.warmup + args.reps):
        lib.check(L.ab_host(ctx._h, C.byref(d), qt.ctypes.data, rq.ctypes.data, len(rq), args.scale, out_h.ctypes.data, ms2, C.byref(by_h)))
        lib.check(L.ab_device(ctx._h, C.byref(b), out_d.ctypes.data, C.byref(ms1), C.byref(by_d)))
        if rep >= args.warmup:
            host.append((ms2[0], ms2[1]))
            dev.append(ms1.value)
    same = out_h.tobytes() == out_d.tobytes()
    rings, pts = ctx.label_tile_batch_expand(gid, qt, rq, args.scale)
    host, dev = np.array(host), np.array(dev)
    doc = {
        "workload": {"tiles": int(len(qt)), "zoom": 15, "requests": int(len(rq)), "rings": int(len(rings)), "points": int(len(pts)), "scale": args.scale,
                     "nodes": int(len(g.nodes))},
        "host_path": {"project_ms_median": float(np.median(host[:, 0])), "label_positions_ms_median": float(np.median(host[:, 1])),
                      "total_ms_median": float(np.median(host.sum(axis=1))), "total_ms_min": float(host.sum(axis=1).min()),
                      "upload_bytes": int(by_h.value)},
        "device_path": {"total_ms_median": float(np.median(dev)), "total_ms_min": float(dev.min()), "upload_bytes": int(by_d.value)},
        "once_per_geodata": {"factors_bytes": int(f.nbytes), "mercator_factors_ms": t_factors * 1e3, "register_ms": t_register * 1e3},
        "speedup_median": float(np.median(host.sum(axis=1)) / np.median(dev)),
        "positions_equal_bit_for_bit": bool(same),
        "statuses": {str(k): int(v) for k, v in zip(*np.unique(out_d["status"], return_counts=True))},
        "reps": args.reps, "warmup": args.warmup,
    }
    if args.kernel_stats:
        doc["kernels"] = kernel_rows(args.kernel_stats)
    ctx.close()
    text = json.dumps(doc, indent=1)
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
