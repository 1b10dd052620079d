"""Label anchors on the GPU (osmt_label_positions): x, y and status of every request compared BIT FOR BIT with the host
mirror (osm_renderer_amd/host/osmt_labelable.hpp through tests/polylabel_shim.cpp), which tests/test_polylabel_cpu.py
ties to an independent Python model.  Runs on poisoned device memory like the rest of the GPU suite (tests/conftest.py)."""
import subprocess

import numpy as np
import pytest

from osm_renderer_amd import abi, labels
from osm_renderer_amd.lib import OsmtError
from tests import _polylabel_model as M
from tests import _polylabel_shim as S

pytestmark = pytest.mark.gpu

LDS_TIER_CELLS = 256  # PL_LDS_CELLS of csrc/osmt_polylabel.hip


def _same(got, want):
    for f in ("x", "y"):
        assert np.array_equal(got[f].view(np.uint64), want[f].view(np.uint64)), f
    assert np.array_equal(got["status"], want["status"])


def _first_diff(got, want):
    bad = np.nonzero((got["x"].view(np.uint64) != want["x"].view(np.uint64)) | (got["y"].view(np.uint64) != want["y"].view(np.uint64))
                     | (got["status"] != want["status"]))[0]
    return None if not len(bad) else (len(bad), int(bad[0]), got[bad[0]], want[bad[0]])


@pytest.fixture(scope="module")
def seeded():
    reqs = M.seeded_requests(20000, seed=7)
    scales = [1.0 if (i // 5) % 2 == 0 else 2.0 for i in range(len(reqs))]
    rings, pts, rq = M.pack(reqs, scales)
    want, peak, pops = S.mirror(rings, pts, rq)
    return rings, pts, rq, want, peak, pops


def test_seeded_families_one_batch(gpu_ctx, seeded):
    rings, pts, rq, want, peak, pops = seeded
    assert len(rq) >= 20000 and set(np.unique(rq["scale"])) == {1.0, 2.0}
    got = gpu_ctx.label_positions(rings, pts, rq)
    assert _first_diff(got, want) is None
    _same(got, want)
    assert not (got["status"] == abi.LABEL_TOO_LARGE).any()
    n, left_lds, too_large = gpu_ctx.label_positions_stats()
    assert n == len(rq) and too_large == 0
    assert left_lds == int((peak > LDS_TIER_CELLS).sum())  # the tiers are as predictable as the answer


@pytest.mark.parametrize("chunk", [4096, 7, 1])
def test_batching_changes_nothing(gpu_ctx, seeded, chunk):
    rings, pts, rq, want, _, _ = seeded
    got = np.zeros(len(rq), labels.LABEL_POSITION_DTYPE)
    for lo in range(0, len(rq), chunk):
        gpu_ctx.label_positions(rings, pts, rq[lo:lo + chunk], out=got[lo:lo + chunk])
    assert _first_diff(got, want) is None
    _same(got, want)


def _ring_of(n_edges, seed):
    rng = np.random.default_rng(seed)
    ang = np.sort(rng.uniform(0, 2 * np.pi, n_edges))
    rad = 100.0 * rng.uniform(0.5, 1.0, n_edges)
    p = np.stack([128.3 + rad * np.cos(ang), 77.7 + rad * np.sin(ang)], 1)
    return np.concatenate([p, p[:1]])


def test_rings_of_64_65_1000_5000_edges(gpu_ctx):
    reqs = [[_ring_of(n, n)] for n in (64, 65, 1000, 5000, 15, 16, 17, 63)]
    # a large outer ring with large inner rings: the multi-ring edge loop and the inside test over many points
    outer = _ring_of(1000, 5)
    c = np.array([128.3, 77.7])
    reqs.append([outer, (c + (outer - c) * 0.3)[::-1].copy(), (c + (_ring_of(65, 9) - c) * 0.1)[::-1].copy()])
    rings, pts, rq = M.pack(reqs, 1.0)
    want, peak, pops = S.mirror(rings, pts, rq)
    got = gpu_ctx.label_positions(rings, pts, rq)
    assert _first_diff(got, want) is None
    assert (got["status"] == abi.LABEL_OK).all()


def _strip(w, h, x0=3.25, y0=-7.5):
    return np.array([[x0, y0], [x0 + w, y0], [x0 + w, y0 + h], [x0, y0 + h], [x0, y0]])


def test_strips_beyond_the_lds_tier_are_answered(gpu_ctx):
    reqs = [[_strip(1000.0, 1.0)], [_strip(3000.0, 0.5)], [_strip(0.25, 4000.0)], [_strip(6000.0, 0.1)], [_strip(65000 / 64.0, 1 / 64.0)],
            [_strip(1024.0, 1 / 64.0)]]  # the last one: exactly 65 536 cells in the queue and 65 536 pops, the cap itself
    rings, pts, rq = M.pack(reqs, 1.0)
    want, peak, pops = S.mirror(rings, pts, rq)
    print("queue peaks", peak.tolist(), "pops", pops.tolist())
    assert ((peak > LDS_TIER_CELLS) & (peak <= abi.LABEL_MAX_CELLS) & (pops <= abi.LABEL_MAX_CELLS)).all()
    assert peak.max() == abi.LABEL_MAX_CELLS and pops.max() == abi.LABEL_MAX_CELLS
    got = gpu_ctx.label_positions(rings, pts, rq)
    assert _first_diff(got, want) is None
    assert (got["status"] == abi.LABEL_OK).all()
    assert gpu_ctx.label_positions_stats() == (len(rq), len(rq), 0)


def test_strip_beyond_the_cap_is_too_large_and_the_collector_falls_back(gpu_ctx):
    # the second one is one cell past the cap: 65 537 cells in the initial grid
    reqs = [[M.square(40)], [_strip(5000.0, 0.01, 0.0, 0.0)], [M.u_shape(86, 103, 10)], [_strip(1024.0 + 1 / 64.0, 1 / 64.0)], [M.square(7)]]
    rings, pts, rq = M.pack(reqs, 1.0)
    want, peak, pops = S.mirror(rings, pts, rq, capped=True)
    assert want["status"].tolist() == [abi.LABEL_OK, abi.LABEL_TOO_LARGE, abi.LABEL_OK, abi.LABEL_TOO_LARGE, abi.LABEL_OK]
    got = gpu_ctx.label_positions(rings, pts, rq)
    assert _first_diff(got, want) is None
    assert got["x"][1] == 0.0 and got["y"][1] == 0.0
    assert gpu_ctx.label_positions_stats()[2] == 2
    # osmt::LabelPositions computes the declined request on the host: the uncapped mirror's answer
    out = subprocess.run([S.build_demo()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[-1] == "fallbacks 1"
    for ln in lines[:-1]:
        i, gs, gx, gy, ws, wx, wy = ln.split()
        assert (gs, gx, gy) == (ws, wx, wy), ln
        assert int(gs) == abi.LABEL_OK


def test_none_and_degenerate_requests(gpu_ctx):
    empty = np.zeros((0, 2))
    reqs = [[], [empty], [empty, M.square(10)], [np.array([[3.5, 4.5]])], [np.array([[1.0, 2.0], [9.0, 2.0], [5.0, 2.0]])], [M.square(10)],
            [M.square(10), empty], [np.array([[0.0, -0.0], [-0.0, 0.0], [0.0, 5.0]])], [np.array([[-0.0, 1.0], [0.0, 1.0], [7.0, 1.0]])]]
    rings, pts, rq = M.pack(reqs, 1.0)
    want, _, _ = S.mirror(rings, pts, rq)
    assert want["status"].tolist()[:3] == [abi.LABEL_NONE] * 3
    got = gpu_ctx.label_positions(rings, pts, rq)
    assert _first_diff(got, want) is None
    assert (got["x"][3], got["y"][3]) == (3.5, 4.5) and (got["x"][4], got["y"][4]) == (1.0, 2.0) and (got["x"][5], got["y"][5]) == (5.0, 5.0)


def test_extreme_coordinates_and_validation(gpu_ctx):
    B = float(2 ** 28)
    d = 5e-324
    reqs = [[np.array([[-B, -B], [B, -B], [B, B], [-B, B], [-B, -B]])],
            [np.array([[B - 8, B - 8], [B, B - 8], [B, B], [B - 8, B], [B - 8, B - 8]])],
            [np.array([[0.0, 0.0], [4 * d, 0.0], [4 * d, 6 * d], [0.0, 6 * d], [0.0, 0.0]])],
            [np.array([[1.0, 1.0], [1.0 + 2 ** -52, 1.0], [1.0 + 2 ** -52, 1.0 + 2 ** -51], [1.0, 1.0 + 2 ** -51], [1.0, 1.0]])],
            [np.array([[0.0, 0.0], [1e-160, 0.0], [1e-160, 1e-160], [0.0, 1e-160], [0.0, 0.0]])]]
    rings, pts, rq = M.pack(reqs, 1.0)
    want, _, _ = S.mirror(rings, pts, rq)
    got = gpu_ctx.label_positions(rings, pts, rq)
    assert _first_diff(got, want) is None
    assert (got["status"] == abi.LABEL_OK).all()
    for bad in (np.nan, np.inf, -np.inf, B + 1.0, -(B + 1.0)):
        p = pts.copy()
        p[7, 1] = bad
        out = np.full(len(rq), 0x5A, np.uint8).view(np.uint8).repeat(24).view(labels.LABEL_POSITION_DTYPE)[:len(rq)].copy()
        before = out.copy()
        with pytest.raises(OsmtError) as e:
            gpu_ctx.label_positions(rings, p, rq, out=out)
        assert e.value.code == abi.UNSUPPORTED
        assert out.tobytes() == before.tobytes()
    for field, val in (("ring_off", len(rings)), ("n_rings", len(rings) + 1)):
        r = rq.copy()
        r[field][1] = val
        with pytest.raises(OsmtError) as e:
            gpu_ctx.label_positions(rings, pts, r)
        assert e.value.code == abi.INVALID_ARG
    rr = rings.copy()
    rr[2, 1] = len(pts)  # a point range past the pool
    with pytest.raises(OsmtError) as e:
        gpu_ctx.label_positions(rr, pts, rq)
    assert e.value.code == abi.INVALID_ARG
    r = rq.copy()
    r["scale"][0] = np.nan
    with pytest.raises(OsmtError) as e:
        gpu_ctx.label_positions(rings, pts, r)
    assert e.value.code == abi.INVALID_ARG
    assert len(gpu_ctx.label_positions(rings, pts, rq[:0])) == 0  # zero requests: OSMT_OK


def test_second_smaller_batch_on_one_context_and_begin_end(gpu_ctx, seeded):
    rings, pts, rq, want, _, _ = seeded
    a = gpu_ctx.label_positions(rings, pts, rq[:3000])
    b = gpu_ctx.label_positions(rings, pts, rq[100:163])  # smaller: a stale workspace would show
    assert _first_diff(a, want[:3000]) is None and _first_diff(b, want[100:163]) is None
    # two jobs in flight, ended in order
    j1 = gpu_ctx.label_positions_begin(rings, pts, rq[:2048])
    j2 = gpu_ctx.label_positions_begin(rings, pts, rq[2048:2100])
    assert _first_diff(gpu_ctx.label_positions_end(j1), want[:2048]) is None
    assert _first_diff(gpu_ctx.label_positions_end(j2), want[2048:2100]) is None
