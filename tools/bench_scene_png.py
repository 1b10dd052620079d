#!/usr/bin/env python
"""PNG files from a resident scene against PNG files from a host-built display list (GPU).

    python tools/bench_scene_png.py [--tiles 1024] [--runs 7] [--warmup 2] [--out profiles/scene_png_bench.json]
    python tools/bench_scene_png.py --device-form            # the workload of the kernel trace, nothing else
    python tools/bench_scene_png.py --merge-stats DIR        # adds the kernel shares of a rocprofv3 --kernel-trace --stats run

Every figure is the median (and the range) of `runs` runs after `warmup` warm-ups; a run ends in a device synchronise (the
host forms return with the files in host memory; a synchronise follows all the same).  Forms that are compared alternate in
one process, and the order flips from run to run.

  scene_vs_batch   osmt_render_scene_png on a resident scene of config-2 tiles against osmt_render_batch_png of the same
                   display list (which validates and uploads it on every call), both into pinned memory
  begin_end        osmt_render_scene_png_begin / osmt_render_batch_png_end over two alternating scenes from one thread, job
                   k + 1 begun before job k is ended, against the same with display lists (osmt_render_batch_png_begin)
  tile_built       tile coordinates to files: osmt_scene_build_tiles, then osmt_render_scene_png
  device_form      osmt_render_scene_png_device between two events on one stream
"""
import argparse
import csv
import glob
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402


def stats(ms):
    ms = [float(v) for v in ms]
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "runs": len(ms)}


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def alternate(forms, runs, warmup, sync):
    """forms: {name: callable}; returns {name: [ms]} with the order flipped from run to run"""
    names = list(forms)
    out = {k: [] for k in names}
    for rep in range(warmup + runs):
        for k in names if rep % 2 == 0 else names[::-1]:
            ms = timed(forms[k], sync)
            if rep >= warmup:
                out[k].append(ms)
    return out


def device_form(ctx, scene, runs, warmup):
    import torch

    png, _, status = ctx.render_scene_png_device(scene)
    ms = []
    for rep in range(warmup + runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ctx.render_scene_png_device(scene, png=png)
        b.record()
        torch.cuda.synchronize()
        if rep >= warmup:
            ms.append(a.elapsed_time(b))
    assert status.cpu().tolist() == [0]
    return ms


def merge_stats(directory, out_path):
    """rocprofv3 --kernel-trace --stats (a rocpd database, or a kernel_stats.csv of older versions): the kernels the device
    form launches and the share of the two new steps"""
    import sqlite3

    dbs = sorted(glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True))
    csvs = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if dbs:
        q = "select name, count(*), sum(duration), avg(duration), min(duration), max(duration) from kernels group by name order by sum(duration) desc"
        rows = [{"name": r[0], "calls": r[1], "total_us": round(r[2] / 1e3, 2), "avg_us": round(r[3] / 1e3, 2), "min_us": round(r[4] / 1e3, 2),
                 "max_us": round(r[5] / 1e3, 2)} for r in sqlite3.connect(dbs[-1]).execute(q)]
    elif csvs:
        raw = list(csv.DictReader(open(csvs[-1])))
        key = next(k for k in raw[0] if "total" in k.lower() and "ns" in k.lower())
        rows = [{"name": r["Name"], "calls": int(r.get("Calls", 0)), "total_us": round(float(r[key]) / 1e3, 2)} for r in raw]
    else:
        raise SystemExit(f"no *_results.db and no *kernel_stats.csv under {directory}")
    ours = [r for r in rows if any(w in r["name"] for w in ("k_png", "k_raster", "k_prebin", "k_sublist", "k_opinfo", "k_project"))]
    for r in ours:
        r["name"] = r["name"][:80]
    total = sum(r["total_us"] for r in ours)
    tail = sum(r["total_us"] for r in ours if "k_png_offsets" in r["name"] or "k_png_compact" in r["name"])
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    res["device_form_kernels"] = {
        "what": "rocprofv3 --kernel-trace --stats over a run of its own (tools/bench_scene_png.py --device-form): the kernels of "
                "osmt_render_scene_png_device; share = k_png_offsets + k_png_compact over all of them",
        "rows": ours,
        "offsets_plus_compact_share": round(tail / total, 5) if total else None,
    }
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res["device_form_kernels"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pipe", type=int, default=8, help="jobs per run of the begin / end leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_png_bench.json"))
    ap.add_argument("--device-form", action="store_true")
    ap.add_argument("--merge-stats", default="")
    ap.add_argument("--no-tile-built", action="store_true")
    args = ap.parse_args()
    if args.merge_stats:
        return merge_stats(args.merge_stats, args.out)

    import torch

    from osm_renderer_amd import styled, synth
    from osm_renderer_amd.lib import load
    from osm_renderer_amd.renderer import Context

    ctx = Context(0)
    sync = torch.cuda.synchronize
    n = args.tiles
    lists = [synth.config2(n), synth.make_tiles(synth.config_tiles(n, x0=21000, y0=11000))]
    scenes = [ctx.upload(dl) for dl in lists]
    if args.device_form:
        ms = device_form(ctx, scenes[0], args.runs, args.warmup)
        print(json.dumps({"device_form": stats(ms)}))
        return
    bound = load().osmt_png_device_bound(256, 256)
    pins = [ctx.host_alloc((n * bound,)) for _ in range(2)]
    res = {"tiles": n, "runs": args.runs, "warmup": args.warmup,
           "what": "wall clock in ms around calls that end in a device synchronise; median and range; forms alternate in one process"}

    # ---- scene form against batch form ----
    t = alternate({"scene": lambda: ctx.render_scene_png(scenes[0], out=pins[0], as_bytes=False),
                   "batch": lambda: ctx.render_batch_png(lists[0], out=pins[1], as_bytes=False)}, args.runs, args.warmup, sync)
    _, off_s = ctx.render_scene_png(scenes[0], out=pins[0], as_bytes=False)
    _, off_b = ctx.render_batch_png(lists[0], out=pins[1], as_bytes=False)
    same = bool(np.array_equal(off_s, off_b) and np.array_equal(pins[0][: int(off_s[-1])], pins[1][: int(off_b[-1])]))
    s, b = stats(t["scene"]), stats(t["batch"])
    res["scene_vs_batch"] = {"scene_form": s, "batch_form": b, "same_files": same, "png_bytes": int(off_s[-1]),
                             "scene_range_at_or_below_or_overlapping_batch_range": bool(s["min_ms"] <= b["max_ms"])}

    # ---- begin / end over two alternating scenes, one thread ----
    def pipe(begin):
        def run():
            prev = begin(0)
            for k in range(1, args.pipe):
                cur = begin(k & 1)
                ctx.png_end(prev, pins[(k - 1) & 1])
                prev = cur
            ctx.png_end(prev, pins[(args.pipe - 1) & 1])
        return run

    t = alternate({"scene": pipe(lambda k: ctx.scene_png_begin(scenes[k])), "batch": pipe(lambda k: ctx.png_begin(lists[k]))}, args.runs, args.warmup, sync)
    res["begin_end"] = {"jobs_per_run": args.pipe, "per_job_scene_form": stats([v / args.pipe for v in t["scene"]]),
                        "per_job_batch_form": stats([v / args.pipe for v in t["batch"]])}

    # ---- the device form, by events ----
    res["device_form"] = dict(stats(device_form(ctx, scenes[0], args.runs, args.warmup)),
                              what="render + encode + k_png_offsets + compaction on one stream, between two events")

    # ---- tile coordinates to files ----
    if not args.no_tile_built:
        from bench_styled_feed import ZOOM, make_world
        from tests import _tilequery as tq
        from tests._geodata import write_geodata
        from tests._styled_feed import recs_of
        from tests.test_styled_builder import _random_styles

        rng = np.random.default_rng(1)
        st, pool = _random_styles(rng, 64)
        nodes, ways, tiles = make_world(n)
        path = os.path.join(tempfile.mkdtemp(prefix="scene_png_"), "world.bin")
        refs = write_geodata(path, nodes, ways, max_zoom_tile=tq.max_zoom_tile)
        gid = ctx.register_geodata(styled.Geodata([[v[1], v[2]] for v in nodes], [(w[0], w[1]) for w in ways]))
        first = ctx.register_styles(recs_of(st), pool)
        ctx.register_tile_index(gid, tq.index_of(refs))
        bid = ctx.register_style_bindings(styled.StyleBindings(gid, 0, 18, [[int(v) + first] for v in rng.integers(0, len(st), len(ways))], []))
        tb = styled.TileBatch(gid, [(z, x, y) for z, x, y, _ in tiles], {ZOOM: bid})
        build, png, both = [], [], []
        for rep in range(args.warmup + args.runs):
            sync()
            t0 = time.perf_counter()
            scene = ctx.build_tiles(tb)
            sync()
            t1 = time.perf_counter()
            _, off = ctx.render_scene_png(scene, out=pins[0], as_bytes=False)
            sync()
            t2 = time.perf_counter()
            scene.free()
            if rep >= args.warmup:
                build.append((t1 - t0) * 1e3), png.append((t2 - t1) * 1e3), both.append((t2 - t0) * 1e3)
        res["tile_built"] = {"build_tiles": stats(build), "render_scene_png": stats(png), "tiles_to_files": stats(both), "png_bytes": int(off[-1]),
                             "what": "config 2's content per tile, 90 ways, queried from the registered index (tools/bench_styled_feed.make_world)"}

    old = json.load(open(args.out)) if os.path.exists(args.out) else {}
    old.update(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(old, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
