#!/usr/bin/env python
"""osmt_build_tile_index on an extract of the size a user registers: what the build costs, where the time goes, and what the
host twin costs on the same input on the same machine (GPU).

    python tools/bench_tile_index_build.py [--ways 300000] [--mps 20000] [--runs 7] [--warmup 2] [--out profiles/tile_index_build_bench.json]

Workload: a seeded synthetic extract — about 2 M nodes; 300 k ways, 99 % of them short walks whose rectangles cover 1 to 4 z18
tiles and 1 % long ones (40 to 200 nodes, rectangles of tens of tiles a side); 20 k multipolygons of one or two small polygons.
The nodes are placed by their Mercator factors over a region of 600 x 600 z18 tiles; every node belongs to one entity.

  build         osmt_build_tile_index with node ids, host clock around the call (it ends in a synchronise), a new geodata id per
                run (one index per file), median (min - max) over the runs after the warm-up
  shares        a child process runs the same builds with OSMT_TRACE_UPLOAD=1 and reports, per build, the device time of the
                sort passes (events around them) and the host time blocked in the read-backs, as shares of the build's time in
                that process (the trace itself costs events, so the shares, not the times, are what to read)
  twin          osmt::tile_index_of on the same input, once (a std::map of std::sets), with the result compared array for array
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def extract(n_ways, n_mps, seed=7):
    """(factors [n, 2], ways, polygons, multipolygons) as lists of node / polygon index ranges"""
    rng = np.random.default_rng(seed)
    W, side, base = float(1 << 18), 600.0, np.array((131000.0, 87000.0))
    long_way = rng.random(n_ways) < 0.01
    n_pts = np.where(long_way, rng.integers(40, 201, n_ways), rng.integers(2, 11, n_ways))
    step = np.where(long_way, 2.0, 0.15)
    poly_of_mp = rng.integers(1, 3, n_mps)
    n_polys = int(poly_of_mp.sum())
    poly_pts = rng.integers(4, 9, n_polys)
    counts = np.concatenate([n_pts, poly_pts])
    starts = np.concatenate([[0], np.cumsum(counts)])
    n_nodes = int(starts[-1])
    owner = np.repeat(np.arange(len(counts)), counts)
    origin = rng.random((len(counts), 2)) * side
    origin[n_ways:] = np.repeat(rng.random((n_mps, 2)) * side, poly_of_mp, axis=0)  # the polygons of a multipolygon lie together
    scale = np.concatenate([step, np.full(n_polys, 0.2)])
    walk = rng.normal(size=(n_nodes, 2)) * scale[owner][:, None]
    walk = np.cumsum(walk, axis=0)
    walk -= walk[starts[:-1]][owner]  # every entity starts at its origin
    t = np.clip(origin[owner] + walk, 0.0, side) + base
    factors = t / W
    way_off = starts[: n_ways + 1].astype(np.uint32)
    poly_off = (starts[n_ways:] - starts[n_ways]).astype(np.uint32)
    mp_off = np.concatenate([[0], np.cumsum(poly_of_mp)]).astype(np.uint32)
    return factors, way_off, poly_off, mp_off


def geodata_of(factors, way_off, poly_off, mp_off):
    from osm_renderer_amd import styled

    g = styled.Geodata.__new__(styled.Geodata)
    n, n_way_nodes = len(factors), int(way_off[-1])
    g.nodes = np.zeros((n, 2))
    g.way_ids = np.arange(len(way_off) - 1, dtype=np.uint64) + np.uint64(5000)
    g.way_node_off, g.way_nodes = way_off, np.arange(n_way_nodes, dtype=np.uint32)
    g.polygon_node_off, g.polygon_nodes = poly_off, np.arange(n_way_nodes, n, dtype=np.uint32)
    g.multipolygon_ids = np.arange(len(mp_off) - 1, dtype=np.uint64) + np.uint64(1 << 33)
    g.multipolygon_polygon_off, g.multipolygon_polygons = mp_off, np.arange(len(poly_off) - 1, dtype=np.uint32)
    return g


def builds(ctx, g, factors, gids, n, sync):
    out, last = [], None
    for _ in range(n):
        gid = ctx.register_geodata(g)
        ctx.register_node_mercator(gid, factors)
        sync()
        t0 = time.perf_counter()
        ctx.build_tile_index(gid, gids)
        out.append((time.perf_counter() - t0) * 1e3)
        last = gid
    return out, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ways", type=int, default=300000)
    ap.add_argument("--mps", type=int, default=20000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_index_build_bench.json"))
    ap.add_argument("--traced-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.environ.setdefault("OSMT_POISON_ALLOC", "0")  # a timing run
    import torch

    from osm_renderer_amd.renderer import Context

    sync = torch.cuda.synchronize
    factors, way_off, poly_off, mp_off = extract(args.ways, args.mps)
    g = geodata_of(factors, way_off, poly_off, mp_off)
    gids = np.arange(len(factors), dtype=np.uint64) + np.uint64(1 << 34)
    ctx = Context(0)
    if args.traced_child:  # the library writes one line per build on stderr
        builds(ctx, g, factors, gids, args.warmup + args.runs, sync)
        ctx.close()
        return
    ms, gid = builds(ctx, g, factors, gids, args.warmup + args.runs, sync)
    from bench_tile_requests import med

    got = ctx.read_tile_index(gid)
    res = {"device": torch.cuda.get_device_name(0),
           "extract": {"nodes": len(factors), "ways": args.ways, "multipolygons": args.mps, "tiles": len(got["tile_xy"]), "way_refs": len(got["ways"]),
                       "multipolygon_refs": len(got["mps"]), "node_refs": len(got["nodes"])},
           "build_ms": med(ms[args.warmup:]), "build_ms_each": [round(v, 3) for v in ms]}
    env = dict(os.environ, OSMT_TRACE_UPLOAD="1")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--traced-child", "--ways", str(args.ways), "--mps", str(args.mps), "--runs", str(args.runs),
                            "--warmup", str(args.warmup)], env=env, capture_output=True, text=True, timeout=900)
    rows = re.findall(r"osmt tile index build: ([0-9.]+) us in all, sort passes ([0-9.]+) us on the device, ([0-9.]+) us of host time blocked in (\d+) read-backs", child.stderr)
    rows = [tuple(float(v) for v in r) for r in rows][args.warmup:]
    if rows:
        res["shares"] = {"sort_passes": med([r[1] / r[0] for r in rows]), "read_back_waits": med([r[2] / r[0] for r in rows]), "read_backs": int(rows[0][3]),
                         "traced_build_ms": med([r[0] / 1e3 for r in rows])}
    else:
        res["shares"] = "not measured: the traced child printed no line (exit %d)" % child.returncode
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from tests import _tileindexbuild as tib

    t0 = time.perf_counter()
    twin = tib.twin_of(g, factors)
    res["twin_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    tib.same(got, twin)
    res["equal_to_twin"] = True
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    main()
