#!/usr/bin/env python
"""Time-boxed fuzz of the label anchors: random request batches through osmt_label_positions against the host mirror
(built with its NaN checks), bit for bit (run on a GPU box, under the poisoned allocator).

    python tools/fuzz_polylabel.py [seconds] [seed]

Families: the seeded ones of tests/_polylabel_model.py (stars, rotated rectangles, L shapes, exactly symmetric integer
shapes, multipolygons with holes / outside rings / empty rings), thin strips that leave the LDS tier, rings of 50 .. 3000
points, tiny and huge extents (1e-300 .. 2^28), coordinates snapped to a coarse grid (ties, collinear and repeated
points).  Prints one line: batches, requests, mismatches, NaN reports of the mirror, requests that left the LDS tier."""
import os
import sys
import time

os.environ.setdefault("OSMT_POISON_ALLOC", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from osm_renderer_amd.renderer import Context  # noqa: E402
from tests import _polylabel_model as M  # noqa: E402
from tests import _polylabel_shim as S  # noqa: E402


def batch(rng, n):
    reqs = M.seeded_requests(n, seed=int(rng.integers(1, 2 ** 31)))
    for _ in range(n // 10):
        k = int(rng.integers(0, 5))
        if k == 0:  # a strip: 300 .. 20 000 cells in the initial grid
            w, h = rng.uniform(300, 3000), rng.uniform(0.15, 1.0)
            x0, y0 = rng.uniform(-100, 100, 2)
            s = np.array([[x0, y0], [x0 + w, y0], [x0 + w, y0 + h], [x0, y0 + h], [x0, y0]])
            reqs.append([s[:, ::-1].copy() if rng.integers(0, 2) else s])
        elif k == 1:
            reqs.append([M.star(rng, int(rng.integers(50, 3000)))])
        elif k == 2:  # extents from denormal-squared to the coordinate bound
            f = 2.0 ** float(rng.integers(-1000, 21))
            reqs.append([(M.star(rng) - 125.0) * f])
        elif k == 3:  # snapped to a grid: repeated points, collinear runs, equal keys
            reqs.append([np.round(M.star(rng, int(rng.integers(5, 40))) / 8.0) * 8.0])
        else:
            reqs.append([np.round(r) for r in M.multipolygon(rng)])
    scales = rng.choice([1.0, 2.0, 1.5], len(reqs))
    return M.pack(reqs, scales)


def main():
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 150.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else int(time.time())
    rng = np.random.default_rng(seed)
    ctx = Context(0)
    t0 = time.time()
    batches = requests = bad = left = too_large = 0
    first = None
    while time.time() - t0 < seconds:
        rings, pts, rq = batch(rng, int(rng.choice([5, 60, 700, 3000])))
        want, _, _ = S.mirror(rings, pts, rq, threads=8)  # asserts the mirror's NaN count is 0
        got = ctx.label_positions(rings, pts, rq)
        st = ctx.label_positions_stats()
        d = np.nonzero((got["x"].view(np.uint64) != want["x"].view(np.uint64)) | (got["y"].view(np.uint64) != want["y"].view(np.uint64))
                       | (got["status"] != want["status"]))[0]
        if len(d) and first is None:
            first = (batches, int(d[0]), got[d[0]], want[d[0]])
        batches, requests, bad, left, too_large = batches + 1, requests + len(rq), bad + len(d), left + st[1], too_large + st[2]
    ctx.close()
    print(f"fuzz_polylabel seed={seed} seconds={seconds:.0f} poison={os.environ.get('OSMT_POISON_ALLOC')}: {batches} batches, {requests} requests, "
          f"{bad} mismatching, mirror NaN reports 0, {left} left the LDS tier, {too_large} too large" + (f"; first mismatch {first}" if first else ""))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
