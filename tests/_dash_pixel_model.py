"""Pixel-local reference of one dashed stroke op, for tiles the CPU oracle cannot render in a test.

The oracle draws a stroke the way line.rs does: it walks EVERY pixel of every edge, on and off the tile, so an edge of
2^29 px at width 65536 is out of reach.  This model evaluates only the tile's pixels.  For each tile pixel and each edge
(p1, p2) of the polyline it computes the inputs that stroke_draw_line (oracle/osm_oracle.cpp, line.rs:65-158) hands to
the calculator:

    center_dist = |numer_const + sdy*x - sdx*y| / denom     (the integer computed exactly, then rounded once)
    long        = point_dist(pixel, p1)
    short       = sqrt(fmax(long^2 - center_dist^2, 0))
    traveled    = sum of point_dist(p1, p2) over the edges before, in order   (draw_lines, line.rs:31)

and runs the oracle's own calculator (oracle_py.opacity_calculate).  A pixel's alpha is initial_opacity * opacity where
is_in_line holds; where several edges reach the same pixel (one generation) the largest alpha wins (tile_pixels.rs:114).

VALIDITY.  This equals the oracle only when every tile pixel in which is_in_line holds is actually VISITED by the
walk, and nothing else is drawn on the tile:
  * every edge whose band (center_dist < feather_to) meets the tile runs far past the tile on BOTH sides along its major
    axis, so each perpendicular run through the tile starts on a centre pixel of the edge and goes on until is_in_line
    fails; an edge whose band misses the tile (a far first edge that only adds to `traveled`) is fine as well;
  * is_in_line must not depend on the dash phase, i.e. cap_dist == 0 for every pixel: the cap used for the dashes is not
    Round (cap NONE / BUTT / SQUARE, or use_caps_for_dashes off), and then a run stops exactly where center_dist reaches
    feather_to;
  * the cap stubs of the first and last point (SQUARE, ROUND) lie far from the tile.
The undashed render of the same op checks the first condition on the GPU; test_dash_pixel_model_matches_the_oracle holds
the model against full oracle renders where those are cheap.
"""
import numpy as np

from osm_renderer_amd import abi


def _point_dist(ax, ay, bx, by):
    dx, dy = float(ax - bx), float(ay - by)
    return float(np.sqrt(dx * dx + dy * dy))


def alpha_plane(points, width, dashes, cap, use_caps_for_dashes, opacity, scale, oracle):
    """(dim, dim) f64 alpha of the op on the tile at global pixels [0, dim) x [0, dim), NaN-free, 0 where nothing is set."""
    cap_for_dashes = cap if use_caps_for_dashes else abi.CAP_NONE
    assert cap_for_dashes != abi.CAP_ROUND, "Round dash caps make is_in_line depend on the phase: the model does not hold"
    dim = 256 * scale
    half_width = width / 2.0
    hlw = float(np.sqrt(half_width * half_width - 0.0 * 0.0))
    feather_to = max(hlw + 0.5, 1.0)
    ys, xs = np.mgrid[0:dim, 0:dim]
    xs = xs.astype(np.int64).ravel()
    ys = ys.astype(np.int64).ravel()
    out = np.zeros(dim * dim, dtype=np.float64)
    traveled = 0.0
    for (x1, y1), (x2, y2) in zip(points[:-1], points[1:]):
        x1, y1, x2, y2 = int(x1), int(y1), int(x2), int(y2)
        if (x1, y1) != (x2, y2):
            numer_const = x2 * y1 - y2 * x1
            sdx, sdy = x2 - x1, y2 - y1
            dxf, dyf = float(abs(sdx)), float(abs(sdy))
            denom = float(np.sqrt(dyf * dyf + dxf * dxf))
            # exact integers: |values| < 2^62 for |coordinates| <= 2^28 (asserted, so int64 cannot wrap)
            assert max(abs(numer_const), abs(sdx), abs(sdy)) < 2**60
            raw = numer_const + sdy * xs - sdx * ys
            cd = np.abs(raw.astype(np.float64)) / denom
            ddx = (xs - x1).astype(np.float64)
            ddy = (ys - y1).astype(np.float64)
            long_d = np.sqrt(ddx * ddx + ddy * ddy)
            short_d = np.sqrt(np.fmax(long_d * long_d - cd * cd, 0.0))
            for i in np.nonzero(cd < feather_to)[0]:
                op, in_line = oracle.opacity_calculate(half_width, dashes, cap_for_dashes, traveled, float(cd[i]), float(short_d[i]))
                if in_line:
                    out[i] = max(out[i], opacity * op)
        traveled += _point_dist(x1, y1, x2, y2)
    return out.reshape(dim, dim)


def expected_canvas(alpha, scale, oracle):
    """(RGBA8, f64 canvas) of a white op with the given alpha plane drawn on canvas=None (black, opaque), through the
    oracle's own set_pixel / blend / to_rgb."""
    px = oracle.Pixels(scale)
    px.reset(None)
    for y, x in zip(*np.nonzero(alpha)):
        a = float(alpha[y, x])
        px.set_pixel(int(x), int(y), (a, a, a, a))
    px.blend_unfinished_pixels()
    f64 = px.pixels_f64()
    rgb = px.to_rgb()
    rgba = np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], axis=-1)
    return rgba, f64
