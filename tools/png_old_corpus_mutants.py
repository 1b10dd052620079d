"""Which deviations of the PNG matcher does a corpus of images tell from the specification?  

Runs tests/_png_model.py with each deviation of tests/test_png_cases_cpu.py::MUTANTS over the 22 images of
tests/test_gpu_png_device.py (test_device_png_matches_model_and_decodes: 6, test_png_fuzz_against_model: 16 — generated here
exactly as there) and over the case corpus of tests/_png_cases.py, and prints per deviation how many images' token streams
differ from the specification's.  Also counts what the matcher met on the old corpus (agreement lengths, symbols, rows per band).
No GPU: `python tools/png_old_corpus_mutants.py`."""
import os
import sys
from collections import Counter

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import _png_cases as C  # noqa: E402
from tests import _png_model as M  # noqa: E402
from tests.test_png_cases_cpu import MUTANTS  # noqa: E402


def old_corpus():
    rng = np.random.default_rng(3)
    imgs = np.zeros((6, 256, 256, 4), dtype=np.uint8)
    imgs[0] = rng.integers(0, 256, size=(256, 256, 4))
    imgs[1, :, :] = (241, 238, 232, 255)
    imgs[2, :, :, :3] = (np.arange(256)[None, :, None] // 3).astype(np.uint8)
    imgs[3, ::2] = 255
    imgs[4, :, :, 0] = rng.integers(0, 2, size=(256, 256)) * 200
    imgs[5, 100:140, 90:200, :3] = rng.integers(140, 256, size=(40, 110, 3))
    imgs[..., 3] = 255
    out = list(imgs)
    rng = np.random.default_rng(2027)
    for W in (256, 512):
        imgs = np.zeros((8, W, W, 4), dtype=np.uint8)
        for im in imgs:
            im[..., :3] = rng.integers(0, 256, size=3)
            for _ in range(int(rng.integers(1, 30))):
                x0, y0 = rng.integers(0, W, size=2)
                w, h = rng.integers(1, W, size=2)
                kind = rng.integers(0, 4)
                sl = (slice(y0, min(W, y0 + h)), slice(x0, min(W, x0 + w)))
                if kind == 0:
                    im[sl][..., :3] = rng.integers(0, 256, size=3)
                elif kind == 1:
                    im[sl][..., :3] = rng.integers(0, 256, size=im[sl][..., :3].shape)
                elif kind == 2:
                    im[sl][..., :3] = (np.arange(im[sl].shape[1])[None, :, None] * int(rng.integers(1, 9))) % 256
                else:
                    im[sl][..., :3] = (np.arange(im[sl].shape[0])[:, None, None] // int(rng.integers(1, 5))) % 256
        imgs[..., 3] = 255
        out += list(imgs)
    return out


def told_apart(images, base):
    res = {}
    for name, rules in MUTANTS.items():
        res[name] = sum(M.tile_tokens(im, rules=dict(M.RULES, **rules))[0] != b for im, b in zip(images, base))
    return res


def main():
    old = old_corpus()
    trace = Counter()
    base = [M.tile_tokens(im, trace=trace)[0] for im in old]
    print("old corpus, %d images: what the matcher met" % len(old))
    for key in ("agree", "taken_len", "len_sym", "dist_sym", "rows_per_band", "rows_up", "window_declined"):
        print("  %-16s %s" % (key, sorted((k[1], v) for k, v in trace.items() if isinstance(k, tuple) and k[0] == key)))
    print("  %s" % {k: v for k, v in trace.items() if not isinstance(k, tuple)})
    print("old corpus: images whose tokens differ under each deviation")
    for name, n in told_apart(old, base).items():
        print("  %-16s %2d of %d%s" % (name, n, len(old), "" if n else "   <- not told apart"))
    new = [c for c in C.all_cases() if c.kind == "matcher"]
    print("case corpus (%d matcher cases): images whose tokens differ under each deviation" % len(new))
    for name, n in told_apart([c.img for c in new], [C.trace(c)[1] for c in new]).items():
        print("  %-16s %2d of %d%s" % (name, n, len(new), "" if n else "   <- not told apart"))


if __name__ == "__main__":
    main()
