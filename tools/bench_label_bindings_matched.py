"""Label bindings per class on the world of tools/bench_selector_match.py: the device calls against the host mirror.

The file of --ways ways and twice as many nodes of the selector-match bench (30 % of the ways carry one of 5000 street names,
the nodes carry no tags), matched against its selector set; every class that matched a selector shows its name under one label
style and an icon-only style without text, every other class nothing.  Reported, each as min / median / max over --runs runs
after --warmup warm-up runs:

  * the whole osmt_register_label_bindings_matched call (nodes) and the whole osmt_register_area_label_bindings_matched call
    (ways + multipolygons): wall clock, registered tags and match, the table left on the device;
  * the device time of their stages, by HIP events, from a child run with OSMT_TRACE_UPLOAD=1;
  * osmt::label_bindings_matched_host / osmt::area_label_bindings_matched_host (host/osmt_selmatch.hpp) on one thread over the
    same input: what the caller's per-entity loop costs;
  * the sizes of the tables, and whether the device's arrays equal the mirror's.

The numbers are the device's and the mirror's own; nothing here is a speed-up promised in advance.

    python tools/bench_label_bindings_matched.py [--ways 1000000] [--selectors 800] [--runs 7] [--warmup 2] [--mirror-runs 1]
                                                 [--out profiles/label_bindings_matched_bench.json]
"""
import argparse
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


from osm_renderer_amd import selmatch, styled  # noqa: E402
from tests import _anchors as an  # noqa: E402
from tests import _labelbind as lb  # noqa: E402
from tests import _selmatch as sm  # noqa: E402
from tests import _tilelabels as tl  # noqa: E402
from tests._geodata import Reader  # noqa: E402

_spec = importlib.util.spec_from_file_location("bench_selector_match", os.path.join(ROOT, "tools", "bench_selector_match.py"))
world = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(world)

STAGES = ("count", "emit", "texts", "measure", "decode", "patch")
PATTERN = re.compile(r"osmt (area label|label) bindings per class: " + ", ".join(rf"{s} ([\d.]+) us" for s in STAGES))


def run(args):
    from osm_renderer_amd.renderer import Context

    tmp = tempfile.mkdtemp(prefix="labelbind_bench_")
    path = os.path.join(tmp, "ways.bin")
    geo, n_tags = world.make_file(path, args.ways)
    r = Reader(path)
    t = sm.TagsOf(r)
    tags = lb.tags_of(t)
    sels = selmatch.SelectorSet(world.make_selectors(args.selectors))
    ctx = Context(0)
    gid = ctx.register_geodata(geo)
    ctx.register_tags(gid, tags)
    ctx.register_tile_index(gid, styled.TileIndex([((0, 0), [], [])]))
    ctx.register_node_mercator(gid, an.mercator_factors(geo.nodes))
    sid = ctx.register_selectors(sels)
    try:
        m = ctx.match_selectors(gid, sid)
    except selmatch.Declined as e:
        m = ctx.match_selectors(gid, sid, sm.host_numbers(t.strings(), e.declined))
    ent, cls, _ = m.read()
    first = ctx.register_label_styles(tl.label_styles([{}, {}]))
    b = selmatch.ClassLabelBindings(0, 18, [[(first, 0), (first + 1, None)] if c["n_sels"] else [] for c in cls], ["name"])
    calls = {"node": m.register_label_bindings, "area": m.register_area_label_bindings}
    call_ms, ids = {k: [] for k in calls}, {}
    for k in range(args.warmup + args.runs):
        for name, call in calls.items():
            t0 = time.perf_counter()
            ids[name] = call(0, 18, b)
            t1 = time.perf_counter()
            if k >= args.warmup:
                call_ms[name].append((t1 - t0) * 1e3)
    if args.child:
        return 0
    got = {"node": ctx.read_label_bindings(ids["node"], r.n_nodes), "area": ctx.read_area_label_bindings(ids["area"], r.n_ways, r.n_multipolygons)}
    mirror_ms, same, sizes = {k: [] for k in calls}, {}, {}
    for name in calls:
        for _ in range(args.mirror_runs):
            t0 = time.perf_counter()
            want = lb.mirror(tags, ent, b, name == "area")
            mirror_ms[name].append((time.perf_counter() - t0) * 1e3)
            arrays = want.arrays() if name == "area" else [want.off[0], want.bind[0], want.text_off, want.chars]
            same[name] = all(a.tobytes() == g.tobytes() for a, g in zip(arrays, got[name]))
        n_bindings = len(got[name][1]) + (len(got[name][3]) if name == "area" else 0)
        sizes[name] = {"bindings": int(n_bindings), "texts": int(len(got[name][-2]) - 1), "chars": int(len(got[name][-1]))}
    # the stages: the same runs in a child with the trace on
    env = dict(os.environ, OSMT_TRACE_UPLOAD="1")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--ways", str(args.ways), "--selectors", str(args.selectors), "--runs", str(args.runs),
           "--warmup", str(args.warmup)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1200)
    stages = {"node": {s: [] for s in STAGES}, "area": {s: [] for s in STAGES}}
    seen = {"node": 0, "area": 0}
    for line in out.stderr.splitlines():
        mm = PATTERN.search(line)
        if not mm:
            continue
        name = "area" if mm.group(1) == "area label" else "node"
        seen[name] += 1
        if seen[name] > args.warmup:  # the warm-up runs left out
            for s, v in zip(STAGES, mm.groups()[1:]):
                stages[name][s].append(float(v))
    res = {
        "what": "osmt_register_label_bindings_matched / osmt_register_area_label_bindings_matched against their host mirrors on one thread, same input",
        "ways": args.ways, "nodes": 2 * args.ways, "tags": n_tags, "selectors": len(sels.selectors), "classes": int(len(cls)),
        "classes_with_bindings": int(sum(1 for c in cls if c["n_sels"])),
        "tables": sizes,
        "device_equals_mirror": same,
        "call_ms": {k: world.spread(v) for k, v in call_ms.items()},
        "device_stage_us": {k: {s: world.spread(v) for s, v in st.items() if v} for k, st in stages.items()},
        "mirror_one_thread_ms": {k: world.spread(v) for k, v in mirror_ms.items() if v},
        "warmup": args.warmup,
    }
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    m.close()
    return 0 if all(same.values()) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ways", type=int, default=1000000)
    ap.add_argument("--selectors", type=int, default=800)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mirror-runs", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_bindings_matched_bench.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    sys.exit(run(ap.parse_args()))


if __name__ == "__main__":
    main()
