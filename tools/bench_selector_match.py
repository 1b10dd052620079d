"""Selector matching on a synthetic file: the device call against the host mirror.

A geodata file of --ways ways (half of them closed, two nodes each) with tags drawn from a key and value pool shaped like OSM
data — a primary tag (highway, building, landuse, natural, waterway), optional name, surface, lanes, maxspeed, width, layer,
bridge, tunnel, oneway — and a selector set of about --selectors selectors built over the same pool the way a stylesheet
repeats its selectors with different zoom ranges and extra tests.  Reported, each as min / median / max over --runs runs
after --warmup warm-up runs:

  * the whole osmt_match_selectors call (wall clock, registered tables, result left on the device);
  * the device time of its stages, by HIP events, from a child run with OSMT_TRACE_UPLOAD=1;
  * osmt::match_selectors_host (host/osmt_selmatch.hpp) on one thread over the same input: what the caller's loop costs
    (--mirror-runs runs; it is slow);
  * the class count, and whether the device's result equals the mirror's.

The numbers are the device's and the mirror's own; nothing here is a speed-up promised in advance.

    python tools/bench_selector_match.py [--ways 1000000] [--selectors 800] [--runs 7] [--warmup 2] [--mirror-runs 1]
                                         [--out profiles/selector_match_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from osm_renderer_amd import abi, selmatch, styled  # noqa: E402
from tests import _selmatch as sm  # noqa: E402
from tests._geodata import Reader  # noqa: E402

A = abi
PRIMARY = {
    "highway": (0.45, ["residential", "service", "track", "footway", "path", "unclassified", "tertiary", "secondary", "primary", "cycleway", "steps", "trunk",
                       "motorway", "living_street", "pedestrian"]),
    "building": (0.38, ["yes", "house", "residential", "garage", "apartments", "industrial", "shed", "roof", "commercial", "retail"]),
    "landuse": (0.07, ["residential", "farmland", "grass", "forest", "meadow", "industrial", "commercial", "cemetery"]),
    "natural": (0.06, ["water", "wood", "scrub", "wetland", "grassland", "beach"]),
    "waterway": (0.04, ["stream", "ditch", "river", "drain", "canal"]),
}
EXTRA = {  # key: (probability, values)
    "bridge": (0.02, ["yes", "viaduct"]),
    "lanes": (0.08, ["1", "2", "3", "4", "6"]),
    "layer": (0.03, ["-1", "1", "2", "0", "-2"]),
    "maxspeed": (0.07, ["30", "50", "60", "80", "100", "30 mph", "signals", "walk"]),
    "name": (0.30, None),  # 5000 street names
    "oneway": (0.06, ["yes", "no", "-1"]),
    "surface": (0.15, ["asphalt", "unpaved", "paved", "gravel", "ground", "concrete", "dirt", "grass"]),
    "tunnel": (0.01, ["yes", "culvert", "building_passage"]),
    "width": (0.03, ["2", "2.5", "3", "3.5", "4.5", "6", "0.5", "1.2 m"]),
}


def make_file(path, n_ways, seed=1):
    """writes the file with numpy (saver.rs's layout, osmt_geodata.hpp has it) and returns styled.Geodata over the same arrays"""
    rng = np.random.default_rng(seed)
    pool, off_of = bytearray(), {}

    def put(s):
        if s not in off_of:
            off_of[s] = (len(pool), len(s.encode()))
            pool.extend(s.encode())
        return off_of[s]

    names = [f"Street {i}" for i in range(5000)]
    keys = sorted(list(PRIMARY) + list(EXTRA))  # ASCII: byte order
    u = rng.random(n_ways)
    edges = np.cumsum([p for p, _ in PRIMARY.values()])
    primary = np.searchsorted(edges, u)  # len(PRIMARY): no primary tag
    present, v_off, v_len = {}, {}, {}
    for k in keys:
        if k in PRIMARY:
            mask, vals = primary == list(PRIMARY).index(k), PRIMARY[k][1]
        else:
            mask, vals = rng.random(n_ways) < EXTRA[k][0], EXTRA[k][1] or names
        table = np.array([put(v) for v in vals], dtype=np.uint32)
        pick = table[rng.integers(0, len(vals), n_ways)]
        present[k], v_off[k], v_len[k] = mask, pick[:, 0], pick[:, 1]
    counts = np.zeros(n_ways, np.int64)
    for k in keys:
        counts += present[k]
    tag_off = np.zeros(n_ways + 1, np.int64)
    tag_off[1:] = np.cumsum(counts)
    quads = np.zeros((int(tag_off[-1]), 4), np.uint32)
    at = tag_off[:-1].copy()
    for k in keys:  # ascending keys: an entity's tags come out sorted
        m = present[k]
        ko, kl = put(k)
        quads[at[m]] = np.stack([np.full(int(m.sum()), ko, np.uint32), np.full(int(m.sum()), kl, np.uint32), v_off[k][m], v_len[k][m]], axis=1)
        at[m] += 1
    # topology: way i = nodes (2i, 2i + 1, then 2i again: closed, or 2i + 1 again: open)
    i = np.arange(n_ways, dtype=np.uint32)
    closed = (i % 2 == 0) & (primary != 0)  # highways stay open
    refs = np.stack([2 * i, 2 * i + 1, np.where(closed, 2 * i, 2 * i + 1)], axis=1).astype(np.uint32)
    nodes = np.zeros(2 * n_ways, np.dtype([("id", "<u8"), ("lat", "<f8"), ("lon", "<f8"), ("t_off", "<u4"), ("t_len", "<u4")]))
    nodes["id"] = np.arange(2 * n_ways) + 1000
    nodes["lat"] = 55.0 + (np.arange(2 * n_ways) % 1000) * 1e-4
    nodes["lon"] = 37.0 + (np.arange(2 * n_ways) // 1000) * 1e-4
    ways = np.zeros(n_ways, np.dtype([("id", "<u8"), ("n_off", "<u4"), ("n_len", "<u4"), ("t_off", "<u4"), ("t_len", "<u4")]))
    ways["id"] = i.astype(np.uint64) + 5000
    ways["n_off"], ways["n_len"] = 3 * i, 3
    ways["t_off"], ways["t_len"] = 3 * n_ways + 4 * tag_off[:-1], 4 * counts
    ints = np.concatenate([refs.reshape(-1), quads.reshape(-1)])
    u32 = lambda v: np.uint32(v).tobytes()
    with open(path, "wb") as f:
        f.write(u32(len(nodes)) + nodes.tobytes() + u32(n_ways) + ways.tobytes() + u32(0) + u32(0) + u32(0) + u32(len(ints)) + ints.tobytes() + bytes(pool))
    g = object.__new__(styled.Geodata)
    g.nodes = np.ascontiguousarray(np.stack([nodes["lat"], nodes["lon"]], axis=1))
    g.way_ids = ways["id"].copy()
    g.way_node_off, g.way_nodes = (3 * np.arange(n_ways + 1)).astype(np.uint32), refs.reshape(-1).copy()
    g.polygon_node_off, g.polygon_nodes = np.zeros(1, np.uint32), np.zeros(0, np.uint32)
    g.multipolygon_ids = np.zeros(0, np.uint64)
    g.multipolygon_polygon_off, g.multipolygon_polygons = np.zeros(1, np.uint32), np.zeros(0, np.uint32)
    return g, int(tag_off[-1])


def make_selectors(n, seed=2):
    """about n selectors over the pools: per primary value a line / area selector, repeated with zoom ranges and extra tests"""
    rng = np.random.default_rng(seed)
    base = []
    for k, (_, vals) in PRIMARY.items():
        typ = A.SEL_WAY if k in ("highway", "waterway") else A.SEL_AREA
        base += [(typ, [(A.TEST_EQUAL, k, v)]) for v in vals]
        base.append((typ, [(A.TEST_EXISTS, k)]))
    extras = [[], [(A.TEST_TRUE, "bridge")], [(A.TEST_TRUE, "tunnel")], [(A.TEST_FALSE, "bridge"), (A.TEST_FALSE, "tunnel")], [(A.TEST_TRUE, "oneway")],
              [(A.TEST_GREATER_OR_EQUAL, "lanes", 3.0)], [(A.TEST_LESS, "width", 3.0)], [(A.TEST_EXISTS, "name")], [(A.TEST_NOT_EQUAL, "surface", "asphalt")],
              [(A.TEST_GREATER, "maxspeed", 50.0)], [(A.TEST_EQUAL, "surface", "unpaved"), (A.TEST_NOT_EXISTS, "name")]]
    out = []
    while len(out) < n:
        typ, tests = base[len(out) % len(base)]
        lo = int(rng.integers(8, 17))
        out.append((typ, tests + extras[int(rng.integers(0, len(extras)))], lo, lo + int(rng.integers(0, 4)) if rng.random() < 0.5 else None))
    out[7] = (A.SEL_NODE, [(A.TEST_EXISTS, "name")], 14, None)
    out[11] = (A.SEL_OTHER, [], None, None)
    return out


def spread(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v), "n": len(v)}


def run(args):
    from osm_renderer_amd.renderer import Context

    tmp = tempfile.mkdtemp(prefix="selmatch_bench_")
    path = os.path.join(tmp, "ways.bin")
    geo, n_tags = make_file(path, args.ways)
    r = Reader(path)
    tags = sm.TagsOf(r)
    sels = selmatch.SelectorSet(make_selectors(args.selectors))
    ctx = Context(0)
    gid = ctx.register_geodata(geo)
    ctx.register_tags(gid, tags.desc())
    sid = ctx.register_selectors(sels)
    ov = None
    try:
        m = ctx.match_selectors(gid, sid)
    except selmatch.Declined as e:
        ov = sm.host_numbers(tags.strings(), e.declined)
        m = ctx.match_selectors(gid, sid, ov)
    got = m.read()
    m.close()
    call_ms = []
    for k in range(args.warmup + args.runs):
        t0 = time.perf_counter()
        m = ctx.match_selectors(gid, sid, ov)
        t1 = time.perf_counter()
        m.close()
        if k >= args.warmup:
            call_ms.append((t1 - t0) * 1e3)
    if args.child:
        return 0
    mirror_ms, same = [], None
    for _ in range(args.mirror_runs):
        t0 = time.perf_counter()
        want = sm.mirror(r, sels)
        mirror_ms.append((time.perf_counter() - t0) * 1e3)
        same = all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    # the stages: the same runs in a child with the trace on
    env = dict(os.environ, OSMT_TRACE_UPLOAD="1")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--ways", str(args.ways), "--selectors", str(args.selectors), "--runs", str(args.runs),
           "--warmup", str(args.warmup)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1200)
    stages = {"tags": [], "count": [], "lists_and_classes": [], "records": []}
    pat = re.compile(r"osmt selector match: tags ([\d.]+) us, count ([\d.]+) us, lists \+ classes ([\d.]+) us, records ([\d.]+) us")
    lines = [mm for mm in (pat.search(line) for line in out.stderr.splitlines()) if mm]
    for mm in lines[1 + args.warmup:]:  # the first call and the warm-up runs left out
        for name, v in zip(stages, mm.groups()):
            stages[name].append(float(v))
    res = {
        "what": "osmt_match_selectors against osmt::match_selectors_host on one thread, same input",
        "ways": args.ways, "nodes": 2 * args.ways, "tags": n_tags, "selectors": len(sels.selectors), "selector_tests": len(sels.tests),
        "declined_values": 0 if ov is None else len(ov),
        "classes": int(len(got[1])), "pooled_selector_ids": int(len(got[2])),
        "device_equals_mirror": same,
        "match_call_ms": spread(call_ms),
        "device_stage_us": {k: spread(v) for k, v in stages.items() if v},
        "mirror_one_thread_ms": spread(mirror_ms) if mirror_ms else None,
        "warmup": args.warmup,
    }
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if same in (True, None) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ways", type=int, default=1000000)
    ap.add_argument("--selectors", type=int, default=800)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mirror-runs", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selector_match_bench.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    sys.exit(run(ap.parse_args()))


if __name__ == "__main__":
    main()
