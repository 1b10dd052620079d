#!/usr/bin/env python
"""Label text as glyph runs against draw_line calls, on the bench's label workload (run on a GPU box).

    python tools/bench_glyph_labels.py [tiles] [labels_per_tile] [steps] [reps]

The workload of bench.py's label_pass leg — 1024 config-2 tiles, 24 labels per tile, 40 % with an icon, 30 % along a
way — built as glyph runs over SYNTH_GLYPHS (labels.make_glyph_labels, a pool of 64 tiles repeated) and expanded on the
host (GlyphLabelList.to_label_list) into the segment form of the same labels.  Prints one JSON line:

  * bytes handed to the library per tile in each form (segments: 40 per label + 32 per draw_line call; runs: 40 per
    label + 64 per glyph instance);
  * the wall time of osmt_scene_set_labels / osmt_scene_set_glyph_labels (median of `reps`) — the segment form's figure
    leaves out the host flattening, which the glyph form does not need (reported separately);
  * the render time with the label pass in each form (HIP events, `steps` renders) and the label pass alone; the two
    must agree within noise: the label kernels read identical calls (checked here).
For the glyph kernels' own time run it under `rocprofv3 --kernel-trace --stats -d <dir> -o glyphs -- python ...`."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from osm_renderer_amd import labels, synth  # noqa: E402
from osm_renderer_amd.renderer import Context  # noqa: E402


def main():
    n_tiles = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    per_tile = int(sys.argv[2]) if len(sys.argv) > 2 else 24
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 7
    ctx = Context(0)
    rng = np.random.default_rng(1)
    sizes = [(16, 16), (12, 20), (20, 20)]
    ids = [ctx.register_image(rng.integers(0, 256, size=(h, w, 4)).astype(np.uint8)) for h, w in sizes]
    table = labels.synth_glyph_table()
    ctx.register_glyphs(table)
    dl = synth.config2(n_tiles)
    pool = min(64, n_tiles)
    base = labels.make_glyph_labels(pool, table, labels_per_tile=per_tile, n_images=3, image_sizes=sizes, seed=2, empty_frac=0.0)
    has_icon = base.labels["has_icon"] == 1
    base.labels["image_id"][has_icon] = np.array(ids, dtype=np.uint32)[base.labels["image_id"][has_icon]]
    gl = base.subset([i % pool for i in range(n_tiles)])
    t0 = time.time()
    base_ll = base.to_label_list(table)
    flatten_s_pool = time.time() - t0
    ll = labels.concat_labels([base_ll.subset([i % pool]) for i in range(n_tiles)])
    scene = ctx.upload(dl)
    out = torch.empty((n_tiles, 256, 256, 4), dtype=torch.uint8, device=ctx.device)

    def timed():
        for _ in range(2):
            ctx.render(scene, out)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            ctx.render(scene, out)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    def set_time(fn, arg):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn(arg)
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3

    ms_plain = timed()
    set_seg_ms = set_time(scene.set_labels, ll)
    ms_seg = timed()
    st_seg = scene.label_status()
    img_seg = out.cpu().numpy()
    set_glyph_ms = set_time(scene.set_glyph_labels, gl)
    ms_glyph = timed()
    st_glyph = scene.label_status()
    img_glyph = out.cpu().numpy()
    segs = scene.read_label_segs()
    same = bool(np.array_equal(segs.view(np.uint64), ll.segs.view(np.uint64)) and np.array_equal(st_seg, st_glyph)
                and np.array_equal(img_seg, img_glyph))
    scene.free()
    ctx.close()
    print(json.dumps({
        "tiles": n_tiles, "labels": int(len(gl.labels)), "glyph_instances": int(len(gl.glyphs)), "draw_line_calls": int(len(ll.segs)),
        "bytes_per_tile_segments": round(ll.algorithmic_bytes() / n_tiles), "bytes_per_tile_glyph_runs": round(gl.input_bytes() / n_tiles),
        "set_labels_ms_segments": round(set_seg_ms, 3), "set_labels_ms_glyph_runs": round(set_glyph_ms, 3),
        "host_flatten_ms_per_tile_python": round(flatten_s_pool / pool * 1e3, 2),
        "ms_areas_only": round(ms_plain, 3), "ms_with_labels_segments": round(ms_seg, 3), "ms_with_labels_glyph_runs": round(ms_glyph, 3),
        "label_pass_ms_segments": round(ms_seg - ms_plain, 3), "label_pass_ms_glyph_runs": round(ms_glyph - ms_plain, 3),
        "identical_calls_pixels_statuses": same,
    }))


if __name__ == "__main__":
    main()
