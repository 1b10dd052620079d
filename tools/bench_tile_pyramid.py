#!/usr/bin/env python
"""The tile index pyramid against the z18 index: what it costs to build, what it holds, what the tile query gains (GPU).

    python tools/bench_tile_pyramid.py [--tiles 1024] [--runs 7] [--warmup 2] [--requests 48] [--out profiles/tile_pyramid_bench.json]

Workload: the world of tools/bench_tile_requests.py (1024 z15 tiles, 92 160 ways, 604 160 nodes, with its node index), in two
contexts of one process: one registers osmt_register_tile_pyramid(OSMT_PYRAMID_ALL_LEVELS), the other does not and runs the
path of the commit before the pyramid — the baseline.

  register      osmt_register_tile_pyramid(ALL_LEVELS), wall time, once per registration of the world (three of them)
  levels        per level its tiles, references per kind and bytes
  zooms 12-18   osmt_scene_build_tiles of a 1024-tile batch (wall ms) and of one tile (p50 over --requests tiles, wall ms) with
                osmt_tile_query_stats beside them.  The tiles of a zoom are the ancestors or the children of the world's z15
                tiles, repeated up to the batch size where a zoom has fewer.  The two forms alternate, the order flips from run
                to run; median (min - max) over the runs.  A build the library refuses is recorded with its message; the batch
                WITHOUT a pyramid is not run where one tile alone gathers more than --batch-limit candidates (its per-tile sort
                runs in device memory and the batch would take minutes): the figure that decided it is recorded.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402


def tiles_of_zoom(z15, zoom, n):
    if zoom <= 15:
        s = 15 - zoom
        t = sorted({(x >> s, y >> s) for _, x, y in z15})
    else:
        s = zoom - 15
        t = [((x << s) + i, (y << s) + j) for _, x, y in z15 for i in range(1 << s) for j in range(1 << s)]
        t = t[:: max(1, len(t) // n)]
    out = [(zoom, x, y) for x, y in t]
    return (out * (n // len(out) + 1))[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--requests", type=int, default=48)
    ap.add_argument("--batch-limit", type=int, default=1 << 16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_pyramid_bench.json"))
    ap.add_argument("--world-cache", default=None)
    args = ap.parse_args()
    if not args.world_cache:
        args.world_cache = tempfile.mkdtemp(prefix="tile_pyramid_")
    os.makedirs(args.world_cache, exist_ok=True)
    os.environ.setdefault("OSMT_POISON_ALLOC", "0")  # a timing run
    import torch

    from bench_tile_requests import med, world
    from osm_renderer_amd import abi, styled
    from osm_renderer_amd.lib import OsmtError
    from osm_renderer_amd.renderer import Context

    sync = torch.cuda.synchronize
    plain, pyr = Context(0), Context(0)
    gid0, bid0, zoom, z15, _, (n_nodes, n_ways), _ = world(plain, args.tiles, args.world_cache)
    res = {"world": {"tiles": len(z15), "ways": n_ways, "nodes": n_nodes, "zoom": zoom}, "device": torch.cuda.get_device_name(0)}
    reg = []
    for _ in range(3):
        gid1, bid1, _, _, _, _, _ = world(pyr, args.tiles, args.world_cache)
        sync()
        t0 = time.perf_counter()
        pyr.register_tile_pyramid(gid1, abi.PYRAMID_ALL_LEVELS)
        reg.append((time.perf_counter() - t0) * 1e3)
    res["register_all_levels_ms"] = {"each": [round(v, 3) for v in reg], "median": round(float(np.median(reg)), 3)}
    res["levels"] = {}
    for lv in range(19):
        a = pyr.read_tile_pyramid(gid1, lv)
        n, cols = len(a["tile_xy"]), len(np.unique(a["tile_xy"][:, 0]))
        words = (2 * cols + 1) + 2 * n + 4 * (n + 1) + len(a["ways"]) + len(a["mps"]) + len(a["nodes"])  # directory, x and y, 3 offsets + zeros, pools
        res["levels"][str(lv)] = {"tiles": n, "way_refs": len(a["ways"]), "multipolygon_refs": len(a["mps"]), "node_refs": len(a["nodes"]), "bytes": 4 * words}
    forms = (("z18_index", plain, gid0, bid0), ("pyramid", pyr, gid1, bid1))

    def build(ctx, gid, bid, tiles):
        sync()
        t0 = time.perf_counter()
        sc = ctx.build_tiles(styled.TileBatch(gid, tiles, {z: bid for z in range(19)}))
        sync()
        ms = (time.perf_counter() - t0) * 1e3
        sc.free()
        return ms

    res["zooms"] = {}
    for z in range(12, 19):
        batch = tiles_of_zoom(z15, z, args.tiles)
        singles = [batch[(i * 131) % len(batch)] for i in range(args.requests)]
        row = {name: {} for name, *_ in forms}
        # one tile first: its counts, and whether the batch without a pyramid is run at all
        run_batch = {}
        for name, ctx, gid, bid in forms:
            try:
                build(ctx, gid, bid, singles[:1])
                row[name]["one_tile_stats"] = ctx.tile_query_stats()
                run_batch[name] = name == "pyramid" or max(row[name]["one_tile_stats"][1:]) <= args.batch_limit
                if not run_batch[name]:
                    row[name]["batch"] = f"not run: one tile gathers {max(row[name]['one_tile_stats'][1:])} candidates"
            except OsmtError as e:
                row[name]["refused"] = str(e)
                run_batch[name] = False
        one = {name: [] for name, *_ in forms}
        bat = {name: [] for name, *_ in forms}
        for rep in range(args.warmup + args.runs):
            for name, ctx, gid, bid in forms if rep % 2 == 0 else forms[::-1]:
                if "refused" in row[name]:
                    continue
                lat = [build(ctx, gid, bid, [t]) for t in singles]
                if run_batch[name]:
                    ms = build(ctx, gid, bid, batch)
                    row[name]["batch_stats"] = ctx.tile_query_stats()
                    if rep >= args.warmup:
                        bat[name].append(ms)
                if rep >= args.warmup:
                    one[name].append(float(np.percentile(lat, 50)))
        for name, *_ in forms:
            if one[name]:
                row[name]["one_tile_p50_ms"] = med(one[name])
            if bat[name]:
                row[name]["batch_ms"] = med(bat[name])
        res["zooms"][str(z)] = row
        print(z, json.dumps(row), flush=True)
    plain.close(), pyr.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
