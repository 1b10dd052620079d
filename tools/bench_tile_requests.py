#!/usr/bin/env python
"""Tile requests: the per-request entry against the three-call chain, the id filter's own cost, and the tile query's stages (GPU).

    python tools/bench_tile_requests.py [--tiles 1024] [--runs 7] [--warmup 2] [--requests 48] [--out profiles/tile_requests_bench.json]
    python tools/bench_tile_requests.py --build-trace      # child mode: the OSMT_TRACE_UPLOAD stage times of osmt_scene_build_tiles, one JSON line
    python tools/bench_tile_requests.py --no-python-threads   # the native threads only

Workload: the world of tools/bench_styled_feed.py (config 2's content per tile: 90 ways of 6 or 7 nodes per z15 tile; at 1024
tiles 92 160 ways and 604 160 nodes), written with its z18 tile index, one style bound to every way, no labels.

  requests_native   T native threads x R one-tile requests, every thread with its own worker handle, through
                osmt_worker_render_tile_png and through the same threads each running the chain it replaces —
                osmt_scene_build_tiles, osmt_render_scene_png, osmt_scene_free (tools/tile_requests_bench.cpp, built and started
                from here over the same world file).  T = 1, 4, 16.  Both forms alternate in one process, the order flips from
                run to run; per form tiles/s of every run and the p50 / p99 of its request latencies: median (min - max) over
                the runs; per thread count the requests and groups the entry counted.  THIS is the figure to quote.
  requests      the same from Python threads, for what a Python server would see.  Every argument of both forms is built
                before the clock starts (a ctypes osmt_tile_batch and osmt_tile_coord per tile); a timed request is one
                ctypes call in the entry form and three in the chain form.  ctypes drops the GIL for the length of a call
                and takes it again between calls, so the chain form passes through the interpreter three times per request
                and the entry form once: the two forms do NOT do equal work under the GIL, and the ratio at many threads
                is not the library's alone.
  filter        osmt_register_id_filter over the whole file (host sort + upload + k_idf_plane for ways and nodes; the planes'
                device time from OSMT_TRACE_UPLOAD=1 in a child run of its own, which registers the filter three times: the first launch of
                the kernel in the process and two warm ones), and osmt_scene_build_tiles of the whole batch
                without a filter against the same with a filter that keeps everything.
  build_trace   the stage times of osmt_scene_build_tiles on the whole batch (OSMT_TRACE_UPLOAD=1, HIP events), medians; run in
                a child process so that OSMT_LIB can point it at another build of the library.
"""
import argparse
import ctypes as C
import json
import os
import pickle
import re
import subprocess
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402


def med(v):
    v = [float(x) for x in v]
    return {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3), "runs": len(v)}


def world(ctx, n_tiles, cache, with_nodes=True):
    """registers the world on ctx; `cache`: a directory that keeps the generated world (and its file) between the processes of a run"""
    from bench_styled_feed import ZOOM, make_world
    from osm_renderer_amd import styled
    from tests import _tilequery as tq
    from tests._geodata import write_geodata

    path, pk = os.path.join(cache, f"world_{n_tiles}.bin"), os.path.join(cache, f"world_{n_tiles}.pickle")
    if os.path.exists(pk) and os.path.exists(path):
        nodes, ways, tiles, refs = pickle.load(open(pk, "rb"))
    else:
        nodes, ways, tiles = make_world(n_tiles)
        refs = write_geodata(path, nodes, ways, max_zoom_tile=tq.max_zoom_tile)
        pickle.dump((nodes, ways, tiles, refs), open(pk, "wb"))
    gid = ctx.register_geodata(styled.Geodata([[v[1], v[2]] for v in nodes], [(w[0], w[1]) for w in ways]))
    st = np.zeros(1, styled.STYLE_REC_DTYPE)
    st["has_fill_color"], st["fill_color"], st["is_foreground_fill"] = 1, (170, 200, 150), 1
    st["has_color"], st["color"], st["has_width"], st["width"] = 1, (70, 70, 90), 1, 1.5
    first = ctx.register_styles(st)
    ctx.register_tile_index(gid, tq.index_of(refs))
    if with_nodes:
        ctx.register_node_index(gid, styled.NodeIndex([v[0] for v in nodes], [sorted(refs[k][0]) for k in sorted(refs)]))
    bid = ctx.register_style_bindings(styled.StyleBindings(gid, 0, 18, [[first] for _ in ways], []))
    every = np.array([v[0] for v in nodes] + [w[0] for w in ways], dtype=np.uint64)
    return gid, bid, ZOOM, [(z, x, y) for z, x, y, _ in tiles], every, (len(nodes), len(ways)), path


def build_trace(args):
    """child mode: stderr of the library is read by the parent; stdout gets one JSON line"""
    from osm_renderer_amd import styled
    from osm_renderer_amd.renderer import Context

    ctx = Context(0)
    gid, bid, zoom, tiles, every, _, _ = world(ctx, args.tiles, args.world_cache)
    tb = styled.TileBatch(gid, tiles, {zoom: bid})
    if args.filter_trace:  # a run of its own: the builds that are compared between two libraries do the same work in both
        for _ in range(3):  # the first launch of k_idf_plane in this process, then warm ones: one trace line each
            ctx.register_id_filter(gid, every)
    for _ in range(args.warmup + args.runs):
        ctx.build_tiles(tb).free()
    ctx.close()
    print(json.dumps({"ok": True}))


def run_build_trace(args, lib=None, filter_trace=False):
    env = dict(os.environ, OSMT_TRACE_UPLOAD="1", OSMT_POISON_ALLOC="0")
    if lib:
        env["OSMT_LIB"] = lib
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--build-trace", "--tiles", str(args.tiles), "--runs", str(args.runs), "--warmup",
                          str(args.warmup), "--world-cache", args.world_cache] + (["--filter-trace"] if filter_trace else []), env=env,
                         capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise RuntimeError(out.stderr[-2000:])
    stages = {}
    lines = [l for l in out.stderr.splitlines() if l.startswith("osmt tile query:")][args.warmup:]
    for l in lines:
        for name, us in re.findall(r"(span|columns|gather|sort|mark \+ scan|emit) ([0-9.]+) us", l):
            stages.setdefault(name, []).append(float(us))
    res = {k: med(v) for k, v in stages.items()}
    res["sum_us"] = med([sum(stages[k][i] for k in stages) for i in range(len(lines))])
    planes = [float(m) for m in re.findall(r"osmt id filter: planes ([0-9.]+) us", out.stderr)]
    if planes:
        res["id_filter_planes_us"] = {"first_launch_in_the_process": planes[0], "warm": planes[1:]}
    return res


def requests(ctx, server, gid, bid, zoom, tiles, threads, n_req, runs, warmup):
    from osm_renderer_amd import abi, styled
    from osm_renderer_amd.lib import check, load

    L = load()
    forms = ("worker_entry", "three_call_chain")
    per = {f: {"tiles_per_s": [], "p50_ms": [], "p99_ms": []} for f in forms}
    workers = [ctx.worker() for _ in range(threads)]
    cap = 1 << 20
    bound = np.empty((threads, cap), np.uint8)
    # every argument of both forms, built before anything is timed
    keep = [styled.TileBatch(gid, [t], {zoom: bid}) for t in tiles]
    structs = [k.as_batch() for k in keep]
    batch_refs = [C.byref(b) for b in structs]
    coords = [abi.TileCoord(int(x), int(y), int(z)) for z, x, y in tiles]
    coord_refs = [C.byref(c) for c in coords]
    outs = [C.c_void_p(bound[t].ctypes.data) for t in range(threads)]
    before = ctx.worker_tile_stats()

    def body(form, t, lat, start):
        w, out, h, sh = workers[t]._h, outs[t], ctx._h, server._h
        got, off, scene = C.c_size_t(), (C.c_uint64 * 2)(), C.c_void_p()
        start.wait()
        for c in range(n_req):
            i = (t * 131 + c * 17) % len(tiles)
            t0 = time.perf_counter()
            if form == "worker_entry":
                rc = L.osmt_worker_render_tile_png(w, sh, coord_refs[i], 1, None, 0, out, cap, C.byref(got))
            else:
                rc = L.osmt_scene_build_tiles(h, batch_refs[i], C.byref(scene))
                if rc == 0:
                    rc = L.osmt_render_scene_png(h, scene, out, cap, off)
                    L.osmt_scene_free(scene)
            lat.append((time.perf_counter() - t0) * 1e3)
            check(rc)

    for rep in range(warmup + runs):
        for form in forms if rep % 2 == 0 else forms[::-1]:
            lats = [[] for _ in range(threads)]
            start = threading.Barrier(threads + 1)
            th = [threading.Thread(target=body, args=(form, t, lats[t], start)) for t in range(threads)]
            for x in th:
                x.start()
            start.wait()
            t0 = time.perf_counter()
            for x in th:
                x.join()
            wall = time.perf_counter() - t0
            if rep >= warmup:
                flat = np.concatenate([np.array(v) for v in lats])
                assert len(flat) == threads * n_req
                per[form]["tiles_per_s"].append(len(flat) / wall)
                per[form]["p50_ms"].append(float(np.percentile(flat, 50)))
                per[form]["p99_ms"].append(float(np.percentile(flat, 99)))
    for w in workers:
        w.close()
    after = ctx.worker_tile_stats()
    res = {f: {k: med(v) for k, v in per[f].items()} for f in forms}
    res["entry_requests"], res["entry_groups"] = after[0] - before[0], after[1] - before[1]  # warm-ups included
    return res


def requests_native(args, world_path, tiles):
    """tools/tile_requests_bench.cpp over the world file: one JSON line per thread count"""
    exe = os.path.join(ROOT, "tests", "_build", "tile_requests_bench")
    src = os.path.join(ROOT, "tools", "tile_requests_bench.cpp")
    libdir = os.path.join(ROOT, "osm_renderer_amd")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(os.path.join(libdir, "libosmtile.so"))):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-o", exe, src, "-L" + libdir, "-losmtile", "-Wl,-rpath," + libdir,
                               "-Wl,-rpath-link,/opt/rocm/lib"])
    import torch

    tf = os.path.join(args.world_cache, "tiles.txt")
    with open(tf, "w") as f:
        f.writelines(f"{z} {x} {y}\n" for z, x, y in tiles)
    env = dict(os.environ, OSMT_POISON_ALLOC="0")
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(os.path.dirname(torch.__file__), "lib"), "/opt/rocm/lib", env.get("LD_LIBRARY_PATH", "")])
    out = subprocess.run([exe, world_path, tf, str(args.runs), str(args.warmup), str(args.requests), "1", "4", "16"], env=env, capture_output=True,
                         text=True, timeout=900)
    if out.returncode != 0:
        raise RuntimeError(out.stderr[-2000:])
    res = {}
    for line in out.stdout.splitlines():
        j = json.loads(line)
        res[str(j["threads"])] = {f: {k: med(v) for k, v in j[f].items()} for f in ("worker_entry", "three_call_chain")}
        res[str(j["threads"])].update(entry_requests=j["entry_requests"], entry_groups=j["entry_groups"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--requests", type=int, default=48)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_requests_bench.json"))
    ap.add_argument("--build-trace", action="store_true")
    ap.add_argument("--no-python-threads", action="store_true")
    ap.add_argument("--filter-trace", action="store_true", help="child mode: register the id filter three times in front of the builds")
    ap.add_argument("--world-cache", default=None, help="a directory for the generated world (default: a fresh temporary one)")
    ap.add_argument("--other-lib", default=None, help="another build of libosmtile.so: its build_trace is measured beside this build's, alternating")
    args = ap.parse_args()
    if not args.world_cache:
        args.world_cache = tempfile.mkdtemp(prefix="tile_requests_")
    os.makedirs(args.world_cache, exist_ok=True)
    if args.build_trace:
        return build_trace(args)
    os.environ.setdefault("OSMT_POISON_ALLOC", "0")  # a timing run
    import torch

    from osm_renderer_amd import styled
    from osm_renderer_amd.renderer import Context

    ctx = Context(0)
    sync = torch.cuda.synchronize
    gid, bid, zoom, tiles, every, (n_nodes, n_ways), world_path = world(ctx, args.tiles, args.world_cache)
    res = {"world": {"tiles": len(tiles), "ways": n_ways, "nodes": n_nodes, "zoom": zoom}, "device": torch.cuda.get_device_name(0)}

    # the filter's own cost
    reg = []
    for rep in range(args.warmup + args.runs):
        t0 = time.perf_counter()
        flt = ctx.register_id_filter(gid, every)
        if rep >= args.warmup:
            reg.append((time.perf_counter() - t0) * 1e3)
    tb = styled.TileBatch(gid, tiles, {zoom: bid})
    t_plain, t_flt = [], []
    for rep in range(args.warmup + args.runs):
        for which in (0, 1) if rep % 2 == 0 else (1, 0):
            sync()
            t0 = time.perf_counter()
            sc = ctx.build_tiles(tb, id_filter=flt if which else None)
            sync()
            ms = (time.perf_counter() - t0) * 1e3
            sc.free()
            if rep >= args.warmup:
                (t_flt if which else t_plain).append(ms)
    res["filter"] = {"register_all_ids_ms": med(reg), "ids": int(len(every)), "build_tiles_unfiltered_ms": med(t_plain),
                     "build_tiles_filter_keeps_everything_ms": med(t_flt)}

    # requests
    server = ctx.tile_server(gid, {zoom: bid})
    res["requests"] = {}
    for threads in () if args.no_python_threads else (1, 4, 16):
        res["requests"][str(threads)] = requests(ctx, server, gid, bid, zoom, tiles, threads, args.requests, args.runs, args.warmup)
    server.close()
    ctx.close()
    res["requests_native"] = requests_native(args, world_path, tiles)

    # the tile query's stages, this build and (optionally) another one, alternating
    traces = {"this": [], "other": []}
    for rep in range(3 if args.other_lib else 1):
        for which in ("this", "other") if rep % 2 == 0 else ("other", "this"):
            if which == "other" and not args.other_lib:
                continue
            traces[which].append(run_build_trace(args, args.other_lib if which == "other" else None))
    res["build_trace"] = {k: v for k, v in traces.items() if v}
    res["filter"]["k_idf_plane_us"] = run_build_trace(args, filter_trace=True)["id_filter_planes_us"]  # a child run of its own

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
