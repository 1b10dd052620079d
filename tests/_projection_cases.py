"""Reader of tests/golden/projection_cases.json (written by tests/golden/make_projection_cases.py from the model of
tests/_projection_model.py).  Needs neither mpmath nor a GPU: the GPU tests read the fixture through it."""
import json
import os
from collections import OrderedDict

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "projection_cases.json")
COLUMNS = ["family", "lat", "lon", "zoom", "tx", "ty", "scale", "x", "y_lo", "y_hi"]
CASE_DTYPE = np.dtype([("family", "U1"), ("lat", "<f8"), ("lon", "<f8"), ("zoom", "<u4"), ("tx", "<u4"), ("ty", "<u4"), ("scale", "<u4"),
                       ("x", "<i4"), ("y_lo", "<i4"), ("y_hi", "<i4")])
_cases = None


def load():
    """every case as one structured array (read once; callers must not write to it)"""
    global _cases
    if _cases is None:
        with open(PATH) as f:
            doc = json.load(f)
        assert doc["columns"] == COLUMNS
        rows = doc["cases"]
        a = np.zeros(len(rows), CASE_DTYPE)
        a["family"] = [r[0] for r in rows]
        for k, name in ((1, "lat"), (2, "lon")):
            a[name] = np.array([int(r[k], 16) for r in rows], np.uint64).view(np.float64)
        for k, name in enumerate(COLUMNS[3:], 3):
            a[name] = [r[k] for r in rows]
        a.setflags(write=False)
        _cases = a
    return _cases


def groups(cases):
    """(zoom, tx, ty, scale) -> indices into `cases`, in first-seen order"""
    out = OrderedDict()
    for i, c in enumerate(cases):
        out.setdefault((int(c["zoom"]), int(c["tx"]), int(c["ty"]), int(c["scale"])), []).append(i)
    return OrderedDict((k, np.array(v)) for k, v in out.items())


def latlon(cases):
    return np.ascontiguousarray(np.stack([cases["lat"], cases["lon"]], axis=1), np.float64)
