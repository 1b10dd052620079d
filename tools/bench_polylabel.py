#!/usr/bin/env python
"""Label anchors: osmt_label_positions against the host mirror on the same requests (run on a GPU box).

    python tools/bench_polylabel.py [tiles] [reps] [--out FILE]

Workload: per tile 64 building-like rings (5 .. 13 points, rotated, non-integer coordinates) and 4 rings of 200 .. 2000
points, scale 1; default 1024 tiles.  Three request sets are timed separately — the buildings, the large rings, both —
because they sit on opposite sides of the yardstick.  Per set, medians of `reps` (>= 7) runs after two untimed ones:

  * call_ms        osmt_label_positions end to end from pageable host arrays: validation, upload, kernels, read-back;
  * mirror_1t_ms / mirror_16t_ms   osm_renderer_amd/host/osmt_labelable.hpp on 1 and on 16 threads of the same machine;
  * left_lds       requests whose queue outgrew the LDS tier (re-run by k_polylabel_big), too_large: declined ones;
  * every answer is compared bit for bit with the mirror first (mismatches must be 0).
Kernel times are not visible from outside the call (it runs on a stream of its own): take them from
`rocprofv3 --kernel-trace --stats -d <dir> -o polylabel -- python tools/bench_polylabel.py <tiles> 3`."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from osm_renderer_amd import labels  # noqa: E402
from osm_renderer_amd.renderer import Context  # noqa: E402
from tests import _polylabel_shim as S  # noqa: E402


def building(rng):
    n = int(rng.integers(4, 13))  # 5 .. 13 points with the closing one
    cx, cy = rng.uniform(0, 256, 2)
    if n == 4:
        a, b = rng.uniform(4, 30, 2)
        q = np.array([[-a, -b], [a, -b], [a, b], [-a, b]]) / 2
    else:
        ang = np.sort(rng.uniform(0, 2 * np.pi, n))
        q = np.stack([np.cos(ang), np.sin(ang)], 1) * (rng.uniform(4, 20) * rng.uniform(0.6, 1.0, n))[:, None]
    t = rng.uniform(0, np.pi)
    c, s = np.cos(t), np.sin(t)
    p = np.stack([cx + q[:, 0] * c - q[:, 1] * s, cy + q[:, 0] * s + q[:, 1] * c], 1)
    return np.concatenate([p, p[:1]])


def large(rng):
    n = int(rng.integers(199, 2000))
    cx, cy = rng.uniform(0, 256, 2)
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    rad = rng.uniform(40, 200) * (0.75 + 0.25 * np.sin(ang * rng.integers(2, 9)) * rng.uniform(0.2, 1.0) + rng.uniform(-0.02, 0.02, n))
    p = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1)
    return np.concatenate([p, p[:1]])


def pack(ring_list):
    n = np.array([len(r) for r in ring_list], np.uint32)
    first = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.uint32)
    rq = np.zeros(len(ring_list), labels.LABEL_REQUEST_DTYPE)
    rq["ring_off"], rq["n_rings"], rq["scale"] = np.arange(len(ring_list)), 1, 1.0
    return np.stack([first, n], 1).astype(np.uint32), np.ascontiguousarray(np.concatenate(ring_list)), rq


def median_ms(f, reps):
    for _ in range(2):
        f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n_tiles = int(args[0]) if len(args) > 0 else 1024
    reps = max(int(args[1]), 3) if len(args) > 1 else 9
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    rng = np.random.default_rng(5)
    pool_b = [building(rng) for _ in range(4096)]
    pool_l = [large(rng) for _ in range(256)]
    b = [pool_b[int(i)] for i in rng.integers(0, len(pool_b), 64 * n_tiles)]
    big = [pool_l[int(i)] for i in rng.integers(0, len(pool_l), 4 * n_tiles)]
    ctx = Context(0)
    res = {"tiles": n_tiles, "reps": reps, "sets": {}}
    for name, ring_list in (("buildings", b), ("large_rings", big), ("both", b + big)):
        rings, pts, rq = pack(ring_list)
        want, peak, pops = S.mirror(rings, pts, rq, threads=16)
        got = ctx.label_positions(rings, pts, rq)
        st = ctx.label_positions_stats()
        bad = int(((got["x"].view(np.uint64) != want["x"].view(np.uint64)) | (got["y"].view(np.uint64) != want["y"].view(np.uint64))
                   | (got["status"] != want["status"])).sum())
        out = np.zeros(len(rq), labels.LABEL_POSITION_DTYPE)
        call = median_ms(lambda: ctx.label_positions(rings, pts, rq, out=out), reps)
        m16 = median_ms(lambda: S.mirror(rings, pts, rq, threads=16), reps)
        m1 = median_ms(lambda: S.mirror(rings, pts, rq, threads=1), max(3, reps // 3))
        res["sets"][name] = {
            "requests": len(rq), "points": int(len(pts)), "mismatches": bad, "left_lds": st[1], "too_large": st[2],
            "left_lds_share": st[1] / len(rq), "pops_mean": float(pops.mean()), "pops_max": int(pops.max()), "queue_peak_max": int(peak.max()),
            "call_ms": call[0], "call_ms_min_max": call[1:], "mirror_16t_ms": m16[0], "mirror_16t_ms_min_max": m16[1:], "mirror_1t_ms": m1[0],
            "device_call_over_mirror_16t": call[0] / m16[0], "requests_per_s_device_call": len(rq) / call[0] * 1e3,
        }
    ctx.close()
    line = json.dumps(res)
    print(line)
    if out_path:
        os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
