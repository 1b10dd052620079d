#!/usr/bin/env python
"""osmt_resolve_refs on an extract of city size: what one resolution costs, where the time goes, where the dedup's two paths
cross, and what the host twin costs on the same input on the same machine (GPU).

    python tools/bench_resolve.py [--nodes 4000000] [--ways 400000] [--runs 5] [--warmup 2] [--out profiles/resolve_bench.json]

Workload: a seeded synthetic extract — node ids ascending with random gaps (2 x a running sum + 1: every node id is odd), in
file order; ways that walk over consecutive nodes from a random start, 90 % of 3 to 20 references, 9.5 % of 20 to 200, 0.5 % of
200 to 2 000, half of them closed (the last reference repeats the first); 1 % of the references step back to the reference
before the last (a repeated pair, which the dedup removes) and 1 % name an even id, which is no node (an extract clipped at its
border); way ids ascending; one relation per 20 ways with 1 to 12 member ways from a random neighbourhood, 3 % of the
members no way.  `seen` is NULL: nodes, then ways, then relations.

  resolution    osmt_resolve_refs + read-back of the counts (not of the arrays), host clock around the call (it ends in a
                synchronise), median (min - max) over the runs after the warm-up, at the library's bound W
  bounds        the same with osmt_debug_resolve_short_way_max at each of --bounds: the measurement W is chosen from
  stages        a child process runs the same resolutions with OSMT_TRACE_UPLOAD=1: the device time of every stage from the
                events around it, medians, per bound
  twin          osmt::resolve_refs_host on the same input, single-threaded, once, with every array compared
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

STAGES = ("id_tables", "translate", "short_ways", "long_ways_mark", "relations_emit")
LINE = (r"osmt id resolution: ([0-9.]+) us in all; id tables ([0-9.]+) us, translate ([0-9.]+) us, short ways ([0-9.]+) us, "
        r"long ways \+ mark ([0-9.]+) us, relations \+ emit ([0-9.]+) us on the device \(.*?, (\d+) pairs through the sort, short way bound (\d+)\)")
BOUNDS = (0, 2, 16, 64, 128, 256, 512, 1024)


def extract(n_nodes, n_ways, seed=9):
    from osm_renderer_amd import styled

    rng = np.random.default_rng(seed)
    node_ids = (2 * np.cumsum(rng.integers(1, 20, n_nodes, dtype=np.int64)) + 1).astype(np.uint64)
    kind = rng.random(n_ways)
    length = np.where(kind < 0.9, rng.integers(3, 21, n_ways), np.where(kind < 0.995, rng.integers(20, 201, n_ways), rng.integers(200, 2001, n_ways))).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(length)])
    total = int(off[-1])
    owner = np.repeat(np.arange(n_ways), length)
    at = np.arange(total) - off[owner]
    start = rng.integers(0, n_nodes, n_ways)
    idx = (start[owner] + at) % n_nodes
    closed = rng.random(n_ways) < 0.5
    last = off[1:] - 1
    idx[last[closed]] = idx[off[:-1][closed]]
    back = np.nonzero((rng.random(total) < 0.01) & (at >= 2))[0]
    idx[back] = idx[back - 2]
    refs = node_ids[idx]
    miss = rng.random(total) < 0.01
    refs[miss] += np.uint64(1)
    way_ids = (np.cumsum(rng.integers(1, 9, n_ways, dtype=np.int64)) + 10).astype(np.uint64)
    n_rels = n_ways // 20
    members = rng.integers(1, 13, n_rels)
    rel_off = np.concatenate([[0], np.cumsum(members)])
    rel_owner = np.repeat(np.arange(n_rels), members)
    near = (rng.integers(0, n_ways, n_rels)[rel_owner] + rng.integers(0, 50, len(rel_owner))) % n_ways
    rel_refs = way_ids[near]
    gone = rng.random(len(rel_refs)) < 0.03
    rel_refs[gone] = np.uint64(5)
    raw = styled.RawOsm([])
    raw.node_ids, raw.way_ids, raw.way_ref_off, raw.way_refs = node_ids, way_ids, off.astype(np.uint32), np.ascontiguousarray(refs)
    raw.relation_ids = np.arange(n_rels, dtype=np.uint64) + np.uint64(1 << 33)
    raw.relation_ref_off, raw.relation_refs = rel_off.astype(np.uint32), np.ascontiguousarray(rel_refs)
    raw.relation_ref_inner = (rng.random(len(rel_refs)) < 0.2).astype(np.uint8)
    return raw


def resolutions(ctx, raw, n, sync):
    """n calls of the C entry and the counts: the arrays stay on the device, as they do for a caller that goes on there"""
    from osm_renderer_amd.lib import check, load

    L, d = load(), raw.as_desc()
    out, counts = [], (C.c_size_t * 5)()
    for _ in range(n):
        sync()
        t0 = time.perf_counter()
        h = C.c_void_p()
        check(L.osmt_resolve_refs(ctx._h, C.byref(d), C.byref(h)))
        check(L.osmt_resolved_counts(h, counts))
        out.append((time.perf_counter() - t0) * 1e3)
        L.osmt_resolved_free(h)
    return out, tuple(int(c) for c in counts)


def traced(args):
    env = dict(os.environ, OSMT_TRACE_UPLOAD="1")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--traced-child", "--nodes", str(args.nodes), "--ways", str(args.ways), "--runs", str(args.runs),
                            "--warmup", str(args.warmup), "--bounds", ",".join(str(b) for b in args.bounds)], env=env, capture_output=True, text=True, timeout=1100)
    rows = [tuple(float(v) for v in r) for r in re.findall(LINE, child.stderr)]
    if not rows:
        return "not measured: the traced child printed no line (exit %d)" % child.returncode
    from bench_tile_requests import med

    out = {}
    for b in args.bounds:
        mine = [r for r in rows if int(r[7]) == b][args.warmup:]
        if not mine:
            continue
        o = {"traced_call_ms": med([r[0] / 1e3 for r in mine]), "pairs_through_the_sort": int(mine[0][6])}
        for k, name in enumerate(STAGES):
            o[name + "_us"] = med([r[1 + k] for r in mine])
        out[str(b)] = o
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=4000000)
    ap.add_argument("--ways", type=int, default=400000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bounds", type=lambda s: tuple(int(v) for v in s.split(",")), default=BOUNDS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resolve_bench.json"))
    ap.add_argument("--traced-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.environ.setdefault("OSMT_POISON_ALLOC", "0")  # a timing run
    import torch

    from osm_renderer_amd.renderer import Context

    sync = torch.cuda.synchronize
    raw = extract(args.nodes, args.ways)
    ctx = Context(0)
    if args.traced_child:  # the library writes one line per resolution on stderr
        for b in args.bounds:
            ctx.debug_resolve_short_way_max(b)
            resolutions(ctx, raw, args.warmup + args.runs, sync)
        ctx.close()
        return
    from bench_tile_requests import med

    n_refs = len(raw.way_refs) + len(raw.relation_refs)
    ms, counts = resolutions(ctx, raw, args.warmup + args.runs, sync)
    got = ctx.resolve_refs(raw)
    res = {"device": torch.cuda.get_device_name(0),
           "extract": {"nodes": len(raw.node_ids), "ways": len(raw.way_ids), "node_references": len(raw.way_refs), "relations": len(raw.relation_ids),
                       "way_references": len(raw.relation_refs), "counts": counts, "ways_longer_than": {str(b): int((np.diff(got["way_node_off"].astype(np.int64)) > b).sum())
                                                                                                    for b in args.bounds}},
           "resolution_ms": med(ms[args.warmup:]), "resolution_ms_each": [round(v, 3) for v in ms]}
    res["references_per_second"] = round(n_refs / (res["resolution_ms"]["median"] / 1e3))
    res["bounds_ms"] = {}
    for b in args.bounds:
        ctx.debug_resolve_short_way_max(b)
        t, c = resolutions(ctx, raw, args.warmup + args.runs, sync)
        assert c == counts, (b, c, counts)
        res["bounds_ms"][str(b)] = med(t[args.warmup:])
    ctx.close()
    res["stages_by_bound"] = traced(args)
    from tests import _resolve as rs

    L, d = rs.shim(), raw.as_desc()
    t0 = time.perf_counter()
    h = L.res_new(C.byref(d))
    res["twin_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    res["twin_references_per_second"] = round(n_refs / (res["twin_ms"] / 1e3))
    try:
        for k, name in enumerate(rs.ARRAYS):
            n = L.res_get(h, k, None, 0)
            a = np.zeros(n, rs.DTYPES.get(name, np.uint32))
            L.res_get(h, k, a.ctypes.data, n)
            assert a.tobytes() == got[name].tobytes(), name
    finally:
        L.res_free(h)
    res["equal_to_twin"] = True
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    main()
