"""The cascade on the world of tools/bench_selector_match.py: the device call against the host mirror.

The same synthetic file (--ways ways, two nodes each) and selector set (about --selectors selectors), with one rule per
selector over three layers ("default", "casing", "labels") and "*": widths, colours, casings, dashes, a text with a font size
on the label layer.  Reported, each as min / median / max over --runs runs after --warmup warm-up runs:

  * the whole osmt_cascade_classes call (wall clock; the result is on the host when it returns);
  * the device time of its stages, by HIP events, from a child run with OSMT_TRACE_UPLOAD=1;
  * osmt_cascade_register for the area tables (styles once, one matched bindings table per zoom range; registrations are
    append-only, so every timed run leaves its tables in the context: --runs bounds what the tool registers);
  * osmt::cascade_host (host/osmt_cascade.hpp) on one thread over the same classes;
  * the counts, and whether the device's arrays equal the mirror's byte for byte.

No threshold: the comparison on record is the device call against the mirror.

--names N (9 .. 255) is the same world with the layers of the casing and label rules drawn from N - 2 names beside "default"
and "*", dealt round so that every name is used; the rules are registered with OSMT_RULES_CLASS_LAYERS, the tool refuses a
world in which a class collects more than 16 layers, and the device time of k_cs_class_layers is reported with the stages.
Its result goes under the key "names_<N>" of the output file, beside the 8-name world's.

    python tools/bench_cascade.py [--ways 1000000] [--selectors 800] [--names N] [--runs 7] [--warmup 2] [--out profiles/cascade_bench.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_selector_match import make_file, make_selectors, spread  # noqa: E402
from osm_renderer_amd import abi, selmatch  # noqa: E402
from tests import _cascade as cs  # noqa: E402
from tests import _selmatch as sm  # noqa: E402
from tests._geodata import Reader  # noqa: E402

A = abi


def make_rules(selectors, sid, names=0):
    """one rule per selector; the layer and the properties follow the selector's number.  names: 0 for the layers "casing" and
    "labels", else the casing and label rules take their layers in turn from names - 2 names"""
    rules, turn = [], 0

    def layer_of(word):
        nonlocal turn
        if not names:
            return word
        turn += 1
        return f"layer{2 + ((turn - 1) * 7) % (names - 2)}"

    for i, s in enumerate(selectors):
        kind = i % 8
        if kind == 0:
            rules.append((["*"], [("linecap", A.PV_IDENTIFIER, "round"), ("opacity", A.PV_NUMBERS, [1.0])]))
        elif kind in (1, 2, 3):
            rules.append(([None], [("color", A.PV_COLOR, (40 + i % 200, 90, 120)), ("width", A.PV_NUMBERS, [1.0 + (i % 7) * 0.5]),
                                   ("fill-color", A.PV_COLOR, (200, 180 + i % 60, 150)), ("z-index", A.PV_NUMBERS, [float(i % 5)])]))
        elif kind in (4, 5):
            rules.append(([layer_of("casing")], [("casing-width", A.PV_WIDTH_DELTA, 1.0), ("casing-color", A.PV_IDENTIFIER, "grey", {"color": (128, 128, 128)}),
                                       ("dashes", A.PV_NUMBERS, [4.0, 2.0 + i % 3])]))
        else:
            rules.append(([layer_of("labels")], [("text", A.PV_IDENTIFIER, "name"), ("font-size", A.PV_NUMBERS, [9.0 + i % 4]), ("text-color", A.PV_COLOR, (0, 0, i % 256)),
                                       ("text-position", A.PV_IDENTIFIER, "line")]))
    return selmatch.RuleSet(sid, rules, 2.0, None, 0)


def run(args):
    from osm_renderer_amd import labels
    from osm_renderer_amd.renderer import Context

    tmp = tempfile.mkdtemp(prefix="cascade_bench_")
    path = os.path.join(tmp, "ways.bin")
    geo, _ = make_file(path, args.ways)
    r = Reader(path)
    tags = sm.TagsOf(r)
    sel_list = make_selectors(args.selectors)
    sels = selmatch.SelectorSet(sel_list)
    ctx = Context(0)
    syn = labels.synth_glyph_table()
    ctx.register_glyphs(syn)
    ctx.register_font(labels.FontTable([(0x41, 1)], [300, 300], [syn.first_id, syn.first_id], []))  # font 0: the label styles name it
    gid = ctx.register_geodata(geo)
    ctx.register_tags(gid, tags.desc())
    sid = ctx.register_selectors(sels)
    rules = make_rules(sel_list, sid, args.names)
    rid = ctx.register_rules(rules, class_layers=bool(args.names))
    ov = None
    try:
        m = ctx.match_selectors(gid, sid)
    except selmatch.Declined as e:
        ov = sm.host_numbers(tags.strings(), e.declined)
        m = ctx.match_selectors(gid, sid, ov)
    _, cls, pooled = m.read()
    layer_of_sel = [b"default" if L == A.LAYER_DEFAULT else bytes(rules.layer_bytes[rules.layer_off[L]:rules.layer_off[L + 1]]) for L in rules.selector_layer.tolist()]
    class_layers = max((len({layer_of_sel[s] for s in pooled[c["sel_off"]:c["sel_off"] + c["n_sels"]]}) for c in cls), default=0)
    if args.names and class_layers > A.CASCADE_MAX_CLASS_LAYERS:
        print(f"a class of this world collects {class_layers} layers (> {A.CASCADE_MAX_CLASS_LAYERS}): choose fewer names", file=sys.stderr)
        return 2
    call_ms, reg_ms, got = [], [], None
    for k in range(args.warmup + args.runs):
        t0 = time.perf_counter()
        c = m.cascade(rid, False)
        t1 = time.perf_counter()
        if got is None:
            got = c.read()
        t2 = time.perf_counter()
        c.register(A.CASCADE_AREA_STYLES)
        t3 = time.perf_counter()
        c.close()
        if k >= args.warmup:
            call_ms.append((t1 - t0) * 1e3)
            reg_ms.append((t3 - t2) * 1e3)
    if args.child:
        return 0
    mirror_ms = []
    for _ in range(args.mirror_runs):
        t0 = time.perf_counter()
        want = cs.mirror(rules, sels, cls, pooled, False)
        mirror_ms.append((time.perf_counter() - t0) * 1e3)
    same = all(a.tobytes() == b.tobytes() for a, b in zip(got.arrays(), want.arrays()))
    env = dict(os.environ, OSMT_TRACE_UPLOAD="1")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--ways", str(args.ways), "--selectors", str(args.selectors), "--runs", str(args.runs),
           "--warmup", str(args.warmup), "--names", str(args.names)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1200)
    stages = {"count_fold_records": [], "distinct": [], "compact_and_zooms": [], "ranges": [], "class_layers": []}
    pat = re.compile(r"osmt cascade: count \+ fold \+ records ([\d.]+) us, distinct ([\d.]+) us, compact \+ zooms ([\d.]+) us, ranges ([\d.]+) us"
                     r".*, class layers ([\d.]+) us")
    lines = [mm for mm in (pat.search(line) for line in out.stderr.splitlines()) if mm]
    for mm in lines[args.warmup:]:
        for name, v in zip(stages, mm.groups()):
            stages[name].append(float(v))
    res = {
        "what": "osmt_cascade_classes against osmt::cascade_host on one thread, same classes",
        "layer_names": len(set(layer_of_sel)), "most_layers_of_a_class": int(class_layers), "class_layers_flag": bool(args.names),
        "ways": args.ways, "selectors": len(sels.selectors), "rules": len(rules.rule_prop_off) - 1, "classes": int(len(cls)),
        "distinct_styles": int(len(got.styles)), "distinct_label_styles": int(len(got.label_styles)), "zoom_ranges": int(len(got.zoom_lo)),
        "class_styles_of_all_ranges": int(len(got.class_styles)), "class_label_bindings_of_all_ranges": int(len(got.bindings)),
        "device_equals_mirror": same,
        "cascade_call_ms": spread(call_ms),
        "device_stage_us": {k: spread(v) for k, v in stages.items() if v},
        "cascade_register_area_styles_ms": spread(reg_ms),
        "mirror_one_thread_ms": spread(mirror_ms),
        "warmup": args.warmup,
    }
    print(json.dumps(res, indent=1))
    if args.names and args.out and os.path.exists(args.out):
        with open(args.out) as f:
            res = dict(json.load(f), **{f"names_{args.names}": res})
    elif args.names:
        res = {f"names_{args.names}": res}
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ways", type=int, default=1000000)
    ap.add_argument("--selectors", type=int, default=800)
    ap.add_argument("--names", type=int, default=0, help="layer names of the sheet (9 .. 255); 0: the 8-name world, no flag")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mirror-runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cascade_bench.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    sys.exit(run(ap.parse_args()))


if __name__ == "__main__":
    main()
