"""tests/_dash_pixel_model.py against full renders of the CPU oracle (no GPU): the model replaces the oracle in
test_gpu_parity_ops.py::test_dash_phase_extreme_coordinates, so it is held bit for bit here, on edges the oracle can
still walk whole (up to ~20 000 px), in eight directions and on the axes, with and without a far first edge."""
import numpy as np
import pytest

from osm_renderer_amd import abi
from osm_renderer_amd.display_list import TileBuilder
from tests import _dash_pixel_model as model

DIRS = [(7, 2), (2, 7), (-2, 7), (-7, 2), (-7, -2), (-2, -7), (2, -7), (7, -2), (1, 0), (0, 1)]
PATTERNS = [
    ([5.0, 3.0], abi.CAP_NONE, False),
    ([0.5, 2.0, 3.0], abi.CAP_BUTT, True),
    ([9.0, 4.0], abi.CAP_SQUARE, True),
    ([0.0, 7.0], abi.CAP_SQUARE, False),
]


def edge_through_tile(d, length, centre=(131, 117)):
    """integer endpoints of an edge of ~length px along direction d through `centre`, plus a far first point whose edge
    to p1 keeps its band away from the tile (it only adds to `traveled`)"""
    n = float(np.hypot(*d))
    ux, uy = d[0] / n, d[1] / n
    h = length / 2.0
    p1 = (int(round(centre[0] - ux * h)), int(round(centre[1] - uy * h)))
    p2 = (int(round(centre[0] + ux * h)), int(round(centre[1] + uy * h)))
    p0 = (int(round(p1[0] - uy * 3000 - ux * 1000)), int(round(p1[1] + ux * 3000 - uy * 1000)))
    return p0, p1, p2


@pytest.mark.parametrize("width", [3.0, 41.0, 301.0])
def test_dash_pixel_model_matches_the_oracle(oracle, width):
    length = {3.0: 20000, 41.0: 6000, 301.0: 1600}[width]
    checked = 0
    for k, d in enumerate(DIRS):
        dashes, cap, ucd = PATTERNS[k % len(PATTERNS)]
        p0, p1, p2 = edge_through_tile(d, length)
        pts = [p0, p1, p2] if k % 2 else [p1, p2]
        for ds in (None, dashes):
            tb = TileBuilder(canvas=None)
            tb.stroke(pts, width, (255, 255, 255), 0.75, dashes=ds, cap=cap, use_caps_for_dashes=ucd)
            want_rgba, want_f64 = oracle.render_job(tb.build(), 0, want_f64=True)
            alpha = model.alpha_plane(pts, width, ds, cap, ucd, 0.75, 1, oracle)
            got_rgba, got_f64 = model.expected_canvas(alpha, 1, oracle)
            same = got_f64.view(np.uint64) == want_f64.view(np.uint64)
            assert same.all(), f"width {width} dir {d} dashes {ds}: f64 differs at {np.argwhere(~same)[0].tolist()}"
            assert np.array_equal(got_rgba, want_rgba)
            checked += int((alpha > 0).sum())
    assert checked > 10000  # the edges do cross the tile
