"""The label-position function on the CPU: the host mirror (osm_renderer_amd/host/osmt_labelable.hpp, built by
tests/polylabel_shim.cpp) against the independent Python model of tests/_polylabel_model.py, bit for bit, plus known
answers and a check that the tie order of the priority queue is observable."""
import ctypes as C

import numpy as np

from osm_renderer_amd import abi, labels
from tests import _polylabel_model as M
from tests import _polylabel_shim as S


def _mirror_one(rings, scale=1.0, capped=True):
    r, p, q = M.pack([rings], scale)
    out, peak, pops = S.mirror(r, p, q, capped=capped)
    return int(out["status"][0]), float(out["x"][0]), float(out["y"][0])


def test_abi_layout_of_the_label_anchor_records():
    s = S.lib().shim_polylabel_sizeof
    assert s(0) == C.sizeof(abi.LabelRequest) == labels.LABEL_REQUEST_DTYPE.itemsize == 16
    assert s(1) == C.sizeof(abi.LabelPosition) == labels.LABEL_POSITION_DTYPE.itemsize == 24
    assert s(2) == C.sizeof(abi.LabelRequestBatch)
    assert s(10) == abi.LabelRequest.scale.offset == labels.LABEL_REQUEST_DTYPE.fields["scale"][1]
    assert s(11) == abi.LabelPosition.status.offset == labels.LABEL_POSITION_DTYPE.fields["status"][1]
    assert s(12) == abi.LabelRequestBatch.points.offset
    assert s(13) == abi.LabelRequestBatch.n_pts.offset
    assert (abi.LABEL_OK, abi.LABEL_NONE, abi.LABEL_TOO_LARGE, abi.LABEL_MAX_CELLS) == (M.OK, M.NONE, M.TOO_LARGE, M.MAX_CELLS)


def test_mirror_equals_the_python_model_bit_for_bit():
    reqs = M.seeded_requests(2500, seed=3)
    scales = np.array([1.0 if (i // 5) % 2 == 0 else 2.0 for i in range(len(reqs))])
    rings, pts, rq = M.pack(reqs, scales)
    out, peak, pops = S.mirror(rings, pts, rq)  # asserts that no NaN reached a minimum or a key
    assert len(rq) >= 2000 and (rq["n_rings"] > 1).sum() >= 400
    for i, r in enumerate(reqs):
        st, x, y, pk, pp = M.label_position([a.tolist() for a in r], float(scales[i]), capped=True)
        got = (int(out["status"][i]), M.bits(out["x"][i]), M.bits(out["y"][i]), int(peak[i]), int(pops[i]))
        assert got == (st, M.bits(x), M.bits(y), pk, pp), (i, i % 5, float(out["x"][i]).hex(), float(x).hex())


def test_known_answers():
    empty = np.zeros((0, 2))
    assert _mirror_one([])[0] == abi.LABEL_NONE
    assert _mirror_one([empty])[0] == abi.LABEL_NONE
    assert _mirror_one([empty, M.square(10)])[0] == abi.LABEL_NONE  # the first ring AS GIVEN, before the filter
    assert _mirror_one([np.array([[3.5, 4.5]])]) == (abi.LABEL_OK, 3.5, 4.5)
    assert _mirror_one([np.array([[9.0, 2.0], [1.0, 2.0], [5.0, 2.0]])]) == (abi.LABEL_OK, 1.0, 2.0)  # zero height: (min_x, min_y)
    assert _mirror_one([M.square(10)]) == (abi.LABEL_OK, 5.0, 5.0)
    assert _mirror_one([M.square(10) + np.array([2.5, -1.25])], 2.0) == (abi.LABEL_OK, 7.5, 3.75)
    # a ring-shaped multipolygon: the answer lies inside the outer ring and outside the hole
    outer = M.square(40)
    hole = (M.square(20) + 10.0)[::-1].copy()
    st, x, y = _mirror_one([outer, hole])
    assert st == abi.LABEL_OK
    assert M.point_dist(x, y, [outer.tolist()]) > 0.0 and M.point_dist(x, y, [hole.tolist()]) < 0.0
    assert M.point_dist(x, y, [outer.tolist(), hole.tolist()]) > 0.0
    assert (x, y) != (20.0, 20.0)
    # a second ring OUTSIDE the first is dropped: same answer as without it
    ell = np.array([[1.5, 2.5], [81.5, 2.5], [81.5, 32.25], [31.75, 32.25], [31.75, 92.5], [1.5, 92.5], [1.5, 2.5]])
    far = M.square(6) + 500.0
    assert _mirror_one([ell, far]) == _mirror_one([ell])
    # ... and so is one that only crosses the boundary
    assert _mirror_one([ell, M.square(6) + np.array([79.0, 0.0])]) == _mirror_one([ell])
    # the larger of two rings leads whichever comes first
    small = M.square(4) + np.array([10.0, 10.0])
    assert _mirror_one([small, ell]) == _mirror_one([ell, small])
    assert _mirror_one([far, ell]) == _mirror_one([ell])
    # the issue's example of the std tie order
    assert _mirror_one([M.u_shape(86, 103, 10)]) == (abi.LABEL_OK, 48.375, 5.375)


def test_caps_are_exact():
    def strip(w, h):
        return np.array([[0.0, 0.0], [w, 0.0], [w, h], [0.0, h], [0.0, 0.0]])

    r, p, q = M.pack([[strip(1024.0, 1 / 64)], [strip(1024.0 + 1 / 64, 1 / 64)], [strip(5000.0, 0.01)]], 1.0)
    out, peak, pops = S.mirror(r, p, q, capped=True)
    assert out["status"].tolist() == [abi.LABEL_OK, abi.LABEL_TOO_LARGE, abi.LABEL_TOO_LARGE]
    assert (int(peak[0]), int(pops[0])) == (65536, 65536)
    out, peak, pops = S.mirror(r, p, q, capped=False)  # the fallback of osmt::LabelPositions: the reference's function
    assert out["status"].tolist() == [abi.LABEL_OK] * 3 and int(peak[2]) > 400000



def test_the_tie_order_is_observable_and_the_mirror_follows_std():
    rng = np.random.default_rng(11)
    shapes = M.symmetric_family(rng, 600)
    rings, pts, rq = M.pack(shapes, 1.0)
    out, _, _ = S.mirror(rings, pts, rq)
    differ = 0
    for i, r in enumerate(shapes):
        ring = [r[0].tolist()]
        st, x, y, _, _ = M.label_position(ring, 1.0, tie="std")
        assert (int(out["status"][i]), M.bits(out["x"][i]), M.bits(out["y"][i])) == (st, M.bits(x), M.bits(y)), i
        _, ox, oy, _, _ = M.label_position(ring, 1.0, tie="other")
        differ += (M.bits(ox), M.bits(oy)) != (M.bits(x), M.bits(y))
    print("shapes whose answer depends on the tie order:", differ, "of", len(shapes))
    assert differ >= 50


def test_denormal_and_extreme_inputs_keep_nans_out_of_the_minimum():
    B = float(2 ** 28)
    d = 5e-324
    reqs = [[np.array([[-B, -B], [B, -B], [B, B], [-B, B], [-B, -B]])],
            [np.array([[0.0, 0.0], [4 * d, 0.0], [4 * d, 6 * d], [0.0, 6 * d], [0.0, 0.0]])],
            [np.array([[0.0, 0.0], [1e-160, 0.0], [1e-160, 1e-160], [0.0, 1e-160], [0.0, 0.0]])],
            [np.array([[1e-170, 3e-165], [7e-162, 1e-170], [5e-163, 8e-162], [1e-170, 3e-165]])]]
    rings, pts, rq = M.pack(reqs, 1.0)
    out, _, _ = S.mirror(rings, pts, rq)  # the shim's NaN count is asserted inside
    for i, r in enumerate(reqs):
        st, x, y, _, _ = M.label_position([a.tolist() for a in r], 1.0, capped=True)  # the model asserts the same
        assert (int(out["status"][i]), M.bits(out["x"][i]), M.bits(out["y"][i])) == (st, M.bits(x), M.bits(y)), i
