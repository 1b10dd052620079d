#!/usr/bin/env python
"""osmt_assemble_multipolygons on an extract of the size a user assembles: what one assembly costs, where the time goes, and
what the host twin costs on the same input on the same machine (GPU).

    python tools/bench_multipolygons.py [--relations 20000] [--runs 7] [--warmup 2] [--out profiles/multipolygons_bench.json]

Workload: a seeded synthetic extract — 20 k relations of one outer ring and, for a third of them, one inner ring; ring lengths
4 to 40 segments for 99.5 % of the rings, 200 to 2 000 for 0.5 %, and one relation whose outer ring has 40 000 segments; rings cut
into ways of 1 to 12 segments, 40 % of the ways reversed, the ways of a relation shuffled; 5 % of the relations damaged (a way
left out).  Several hundred thousand segments.

  assembly      osmt_assemble_multipolygons + read-back of the counts, host clock around the call (it ends in a synchronise),
                median (min - max) over the runs after the warm-up
  stages        a child process runs the same assemblies with OSMT_TRACE_UPLOAD=1: the device time of every stage from the
                events around it, medians
  variant       --variant NAME: the same child once more over osm_renderer_amd/libosmtile_NAME.so (build.build_variant), to set
                another build of the walk beside this one — how the LDS staging was measured before it was dropped
  twin          osmt::assemble_multipolygons_host on the same input, single-threaded, once, with every array compared
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

STAGES = ("count", "segments_vertices", "sort", "adjacency_walk", "emit")
LINE = (r"osmt multipolygon assembly: ([0-9.]+) us in all; count ([0-9.]+) us, segments \+ vertices ([0-9.]+) us, sort ([0-9.]+) us, "
        r"adjacency \+ walk ([0-9.]+) us, emit ([0-9.]+) us")


def extract(n_relations, seed=9):
    from osm_renderer_amd import styled

    rng = np.random.default_rng(seed)
    way_off, way_nodes, rel_off, rel_ways, rel_inner = [0], [], [0], [], []
    n_nodes = 0
    for r in range(n_relations):
        members = []
        for role in ((0, 1) if rng.random() < 1 / 3 else (0,)):
            n = int(rng.integers(200, 2001)) if rng.random() < 0.005 else int(rng.integers(4, 41))
            if r == n_relations // 2 and role == 0:
                n = 40000
            ring = np.arange(n_nodes, n_nodes + n + 1, dtype=np.uint32)
            ring[-1] = n_nodes
            n_nodes += n
            at = 0
            while at < n:
                k = min(int(rng.integers(1, 13)), n - at)
                way = ring[at:at + k + 1]
                members.append((len(way_off) - 1, role))
                way_nodes.append(way[::-1] if rng.random() < 0.4 else way)
                way_off.append(way_off[-1] + k + 1)
                at += k
        order = rng.permutation(len(members))
        if rng.random() < 0.05:
            order = order[1:]
        rel_ways += [members[i][0] for i in order]
        rel_inner += [members[i][1] for i in order]
        rel_off.append(len(rel_ways))
    rel = styled.Relations(np.zeros((0, 2)))
    # every node a position of its own: (index, 0.5) is exact in a double
    rel.nodes = np.stack([np.arange(n_nodes, dtype=np.float64), np.full(n_nodes, 0.5)], axis=1)
    rel.way_node_off, rel.way_nodes = np.array(way_off, np.uint32), np.concatenate(way_nodes).astype(np.uint32)
    rel.relation_ids = np.arange(n_relations, dtype=np.uint64) + np.uint64(1 << 33)
    rel.relation_way_off, rel.relation_ways, rel.relation_way_inner = np.array(rel_off, np.uint32), np.array(rel_ways, np.uint32), np.array(rel_inner, np.uint8)
    return rel


def assemblies(ctx, rel, n, sync):
    out, last = [], None
    for _ in range(n):
        sync()
        t0 = time.perf_counter()
        last = ctx.assemble_multipolygons(rel)
        out.append((time.perf_counter() - t0) * 1e3)
    return out, last


def traced(args, lib_path=None):
    env = dict(os.environ, OSMT_TRACE_UPLOAD="1")
    if lib_path:
        env["OSMT_LIB"] = lib_path
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--traced-child", "--relations", str(args.relations), "--runs", str(args.runs), "--warmup",
                            str(args.warmup)], env=env, capture_output=True, text=True, timeout=900)
    rows = [tuple(float(v) for v in r) for r in re.findall(LINE, child.stderr)][args.warmup:]
    if not rows:
        return "not measured: the traced child printed no line (exit %d)" % child.returncode
    from bench_tile_requests import med

    out = {"traced_call_ms": med([r[0] / 1e3 for r in rows])}
    for k, name in enumerate(STAGES):
        out[name + "_us"] = med([r[1 + k] for r in rows])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--relations", type=int, default=20000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multipolygons_bench.json"))
    ap.add_argument("--variant", default="")
    ap.add_argument("--traced-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.environ.setdefault("OSMT_POISON_ALLOC", "0")  # a timing run
    import torch

    from osm_renderer_amd.renderer import Context

    sync = torch.cuda.synchronize
    rel = extract(args.relations)
    ctx = Context(0)
    if args.traced_child:  # the library writes one line per assembly on stderr
        assemblies(ctx, rel, args.warmup + args.runs, sync)
        ctx.close()
        return
    ms, got = assemblies(ctx, rel, args.warmup + args.runs, sync)
    ctx.close()
    from bench_tile_requests import med

    st = got["status"]
    res = {"device": torch.cuda.get_device_name(0),
           "extract": {"relations": args.relations, "nodes": len(rel.nodes), "ways": len(rel.way_node_off) - 1, "segments": int(len(rel.way_nodes) - (len(rel.way_node_off) - 1)),
                       "accepted": int(st["accepted"].sum()), "polygons": len(got["polygon_node_off"]) - 1, "polygon_nodes": len(got["polygon_nodes"])},
           "assembly_ms": med(ms[args.warmup:]), "assembly_ms_each": [round(v, 3) for v in ms]}
    res["stages"] = traced(args)
    if args.variant:
        variant = os.path.join(ROOT, "osm_renderer_amd", f"libosmtile_{args.variant}.so")
        res["stages_of_variant_" + args.variant] = traced(args, variant) if os.path.exists(variant) else "not measured: the variant library is not built"
    from tests import _polygons as mp

    L, d = mp.shim(), rel.as_desc()
    t0 = time.perf_counter()
    h = L.mpa_new(C.byref(d))
    res["twin_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    try:
        for k, name in enumerate(mp.ARRAYS):
            n = L.mpa_get(h, k, None, 0)
            a = np.zeros(n, mp.DTYPES.get(name, np.uint32))
            L.mpa_get(h, k, a.ctypes.data, n)
            assert a.tobytes() == got[name].tobytes(), name
    finally:
        L.mpa_free(h)
    res["equal_to_twin"] = True
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    main()
