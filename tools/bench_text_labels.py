#!/usr/bin/env python
"""Label text as text runs against glyph runs, on the bench's label workload (run on a GPU box).

    python tools/bench_text_labels.py [tiles] [labels_per_tile] [reps]

1024 config-2 tiles x 24 labels from labels.make_text_labels (a pool of 64 tiles repeated): what TextPlacer::place is
given.  The glyph-run form of the same labels is the placement of tests/_text_placer_model.py.  Prints one JSON line:

  * bytes handed to the library per tile in each form — arithmetic, not a measurement: text runs 40 + 64 per label,
    16 per glyph, 24 per way point; glyph runs 40 per label + 64 per glyph instance;
  * the wall time of osmt_scene_set_glyph_labels and osmt_scene_set_text_labels: 2 untimed calls, then the median, the
    minimum and the maximum of `reps` (7) calls, in this process, one after the other; the host-only
    osmt_validate_text_labels (which every text set call runs first) the same way;
  * whether the two forms gave identical draw_line calls, pixels and statuses;
  * the string form (labels.make_string_labels: the same labels as code points and a font size, the font registered once)
    against the text form of the same labels: bytes per tile (40 + 64 per label, 4 per char, 24 per way point; the font
    tables are handed over once per context, not per tile), and the wall time of osmt_scene_set_string_labels and
    osmt_scene_set_text_labels called ALTERNATELY — 2 untimed pairs, then `reps` pairs — as median, minimum and maximum
    each, the host-only osmt_validate_string_labels the same way, and whether shaped records, glyph instances,
    draw_line calls, pixels and statuses are identical.
For k_text_shape's and k_text_place's own time run it under `rocprofv3 --kernel-trace --stats -d <dir> -o text -- python ...`."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from osm_renderer_amd import abi, labels, synth  # noqa: E402
from osm_renderer_amd.lib import load  # noqa: E402
from osm_renderer_amd.renderer import Context  # noqa: E402
from tests import _text_placer_model as model  # noqa: E402


def main():
    n_tiles = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    per_tile = int(sys.argv[2]) if len(sys.argv) > 2 else 24
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    ctx = Context(0)
    rng = np.random.default_rng(1)
    sizes = [(16, 16), (12, 20), (20, 20)]
    ids = [ctx.register_image(rng.integers(0, 256, size=(h, w, 4)).astype(np.uint8)) for h, w in sizes]
    table = labels.synth_glyph_table()
    ctx.register_glyphs(table)
    dl = synth.config2(n_tiles)
    pool = min(64, n_tiles)
    base = labels.make_text_labels(pool, table, labels_per_tile=per_tile, n_images=3, image_sizes=sizes, seed=2)
    has_icon = base.labels["has_icon"] == 1
    base.labels["image_id"][has_icon] = np.array(ids, dtype=np.uint32)[base.labels["image_id"][has_icon]]
    idx = [i % pool for i in range(n_tiles)]
    tl = base.subset(idx)
    gl = model.place_text_labels(base).subset(idx)
    scene = ctx.upload(dl)
    out = torch.empty((n_tiles, 256, 256, 4), dtype=torch.uint8, device=ctx.device)

    def set_times(fn, arg):
        for _ in range(2):
            fn(arg)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn(arg)
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median": round(float(np.median(ts)), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}

    def result():
        ctx.render(scene, out)
        torch.cuda.synchronize()
        return scene.read_label_segs(), scene.label_status(), out.cpu().numpy()

    tb = tl.as_batch()
    validate_ms = set_times(lambda b: load().osmt_validate_text_labels(C.byref(b), n_tiles), tb)  # host only: part of every set call
    glyph_ms = set_times(scene.set_glyph_labels, gl)
    segs_g, st_g, img_g = result()
    text_ms = set_times(scene.set_text_labels, tl)
    inst = scene.read_glyph_instances()
    segs_t, st_t, img_t = result()
    glyph_again_ms = set_times(scene.set_glyph_labels, gl)
    same = bool(np.array_equal(segs_g.view(np.uint64), segs_t.view(np.uint64)) and np.array_equal(st_g, st_t) and np.array_equal(img_g, img_t))

    # the string form against the text form of the same labels, alternately
    kw = dict(labels_per_tile=per_tile, n_images=3, image_sizes=sizes, seed=2)
    sbase, font = labels.make_string_labels(pool, table, **kw)
    ctx.register_font(font)
    sbase.with_font(font)
    tbase = labels.make_text_labels(pool, table, f32_scale=True, **kw)
    for x in (sbase, tbase):
        x.labels["image_id"][has_icon] = np.array(ids, dtype=np.uint32)[x.labels["image_id"][has_icon]]
    sl, tl32 = sbase.subset(idx), tbase.subset(idx)
    sb = sl.as_batch()
    validate_s_ms = set_times(lambda b: load().osmt_validate_string_labels(C.byref(b), n_tiles, ctx._h), sb)
    ts_text, ts_str = [], []
    for rep in range(reps + 2):
        for fn, arg, ts in ((scene.set_text_labels, tl32, ts_text), (scene.set_string_labels, sl, ts_str)):
            t0 = time.perf_counter()
            fn(arg)
            if rep >= 2:
                ts.append((time.perf_counter() - t0) * 1e3)

    def stats(ts):
        return {"median": round(float(np.median(ts)), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}

    recs, inst_s = scene.read_text_glyphs(), scene.read_glyph_instances()
    segs_s, st_s, img_s = result()
    scene.set_text_labels(tl32)
    inst_t = scene.read_glyph_instances()
    segs_t2, st_t2, img_t2 = result()
    same_s = bool(np.array_equal(recs.view(np.uint8), tl32.glyphs.view(np.uint8)) and np.array_equal(inst_s.view(np.uint8), inst_t.view(np.uint8))
                  and np.array_equal(segs_s.view(np.uint64), segs_t2.view(np.uint64)) and np.array_equal(st_s, st_t2) and np.array_equal(img_s, img_t2))
    text_alt, str_alt = stats(ts_text), stats(ts_str)
    scene.free()
    ctx.close()
    print(json.dumps({
        "tiles": n_tiles, "labels": int(len(tl.labels)), "text_glyphs": int(len(tl.glyphs)), "way_points": int(len(tl.way_pts)),
        "glyph_instances_placed": int((inst["form"] != abi.GLYPH_NONE).sum()), "glyph_instances_skipped": int((inst["form"] == abi.GLYPH_NONE).sum()),
        "draw_line_calls": int(len(segs_t)),
        "bytes_per_tile_text_runs": round(tl.input_bytes() / n_tiles), "bytes_per_tile_glyph_runs": round(gl.input_bytes() / n_tiles),
        "bytes_per_tile_glyph_runs_all_glyphs": round((40 * len(tl.labels) + 64 * len(tl.glyphs) + 4 * len(tl.job_label_off)) / n_tiles),
        "set_glyph_labels_ms": glyph_ms, "set_text_labels_ms": text_ms, "set_glyph_labels_ms_again": glyph_again_ms,
        "validate_text_labels_ms": validate_ms,
        "text_minus_glyph_median_ms": round(text_ms["median"] - glyph_ms["median"], 3),
        "glyph_min_max_spread_ms": round(glyph_ms["max"] - glyph_ms["min"], 3),
        "identical_calls_pixels_statuses": same,
        "chars": int(len(sl.chars)), "font_glyphs": int(len(font.advance)), "font_cmap_entries": int(len(font.cmap)), "font_kern_pairs": int(len(font.kern)),
        "font_bytes_once": int(8 * len(font.cmap) + 8 * len(font.advance) + 12 * len(font.kern) + 16),
        "bytes_per_tile_strings": round(sl.input_bytes() / n_tiles), "bytes_per_tile_text_runs_same_labels": round(tl32.input_bytes() / n_tiles),
        "set_text_labels_ms_alternating": text_alt, "set_string_labels_ms_alternating": str_alt,
        "validate_string_labels_ms": validate_s_ms,
        "string_minus_text_median_ms": round(str_alt["median"] - text_alt["median"], 3),
        "text_min_max_spread_ms": round(text_alt["max"] - text_alt["min"], 3),
        "string_identical_records_instances_calls_pixels_statuses": same_s,
    }))


if __name__ == "__main__":
    main()
