"""The scan between the glyph passes (k_glyph_scan_blocks / k_glyph_scan_top, osmt_glyphs.hip) at its edges.

Every (label, glyph) pair's draw_line count is scanned in blocks of 1024 pairs, and the block totals by ONE workgroup
that loops with a carry once there are more than 1024 blocks, i.e. more than 1024^2 pairs — a 10 000-tile batch with 24
labels of ten glyphs has 2.4 M.  Pair counts: 1, one block short of / exactly / one over full (1023, 1024, 1025), two
blocks and a third (2047, 2049), and 1024^2 + 1025, where the carry loop runs a second, partial round of two blocks.

The labels name overlapping ranges of a table of 300 instances, most of them the shapeless glyph with an irregular
sprinkling of a triangle (three calls), so the arena stays small.  Expected arena: every distinct instance expanded once
with the host twin (labels.glyph_segments), assembled with numpy indexing; compared bit for bit with
osmt_scene_read_label_segs.  Each label's n_segs / seg_off (host sums of the count pass's read-back) must name exactly
its calls in that arena: after a render the planes of a sample of labels — the first, the last, those around the pair
1024^2 — hold the oracle's bits for the expected calls of that label."""
import numpy as np
import pytest

from osm_renderer_amd import abi, labels
from osm_renderer_amd.display_list import TileBuilder
from tests import _label_cover_cases as lc

N_INST = 300
TRIANGLE = [("M", 0, 0, 0, 0), ("L", 300, 500, 0, 0), ("L", 600, 0, 0, 0), ("L", 0, 0, 0, 0)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def table(gpu_ctx):
    t = labels.GlyphTable([[], TRIANGLE])
    gpu_ctx.register_glyphs(t)
    return t


def _instances(table):
    """(instances, calls [N_INST, 3, 4] of the host twin, count [N_INST] in {0, 3})"""
    rng = np.random.default_rng(77)
    inst = np.zeros(N_INST, labels.GLYPH_INSTANCE_DTYPE)
    tri = rng.random(N_INST) < 0.12
    tri[[0, 5, 6, 7, 130, 299]] = True
    inst["glyph_id"] = table.first_id + tri.astype(np.uint32)
    inst["form"] = abi.GLYPH_CENTER
    inst["scale"] = 0.002
    inst["p"][:, 0] = 100.0 + 8.0 * rng.random(N_INST)
    inst["p"][:, 1] = 60.0 + 8.0 * rng.random(N_INST)
    calls = np.zeros((N_INST, 3, 4))
    for i in np.nonzero(tri)[0]:
        out = labels.glyph_segments(table.outline(int(inst["glyph_id"][i])), float(inst["scale"][i]),
                                    labels.center_tr(float(inst["p"][i, 0]), float(inst["p"][i, 1])), [])
        calls[i] = np.array(out)
    return inst, calls, 3 * tri.astype(np.int64)


def _labels(n_pairs, seed):
    """Labels with text naming ranges of the instance table, n_pairs instances in all; now and then a label without
    text or with no glyph (no pair).  Returns (label records, and of the labels with pairs: index, range start, range
    length)."""
    rng = np.random.default_rng(seed)
    lens = []
    left = n_pairs
    while left:
        n = int(min(left, rng.integers(1, 257)))
        lens.append(n)
        left -= n
    lens = np.array(lens, dtype=np.int64)
    offs = (rng.random(len(lens)) * (N_INST - lens + 1)).astype(np.int64)
    if n_pairs == 1:
        offs[0] = 5  # a triangle: the one pair draws
    n_lab = len(lens) + len(lens) // 50 + 2
    lab = np.zeros(n_lab, labels.LABEL_DTYPE)
    slot = np.sort(rng.choice(n_lab, len(lens), replace=False))
    lab["has_text"][slot] = 1
    lab["seg_off"][slot] = offs
    lab["n_segs"][slot] = lens
    rest = np.setdiff1d(np.arange(n_lab), slot)
    lab["has_text"][rest[::2]] = 1  # a text of zero glyphs; the others have no text at all
    return lab, slot, offs, lens


def _case(table, n_pairs):
    """(GlyphLabelList, expected arena, and of the labels with pairs: index, first call, calls, first pair)"""
    inst, calls, cnt = _instances(table)
    lab, slot, offs, lens = _labels(n_pairs, 1000 + n_pairs % 997)
    assert int(lab["n_segs"][lab["has_text"] == 1].sum()) == n_pairs
    gl = labels.GlyphLabelList(lab, [0, len(lab)], inst)
    # expected arena: the pairs in label order, each the calls of its instance
    pair_inst = np.concatenate([np.arange(o, o + n) for o, n in zip(offs, lens)])
    draws = cnt[pair_inst] > 0
    want = calls[pair_inst[draws]].reshape(-1, 4)
    csum = np.concatenate([[0], np.cumsum(cnt)])
    lab_n = csum[offs + lens] - csum[offs]  # calls of every label with pairs
    lab_off = np.concatenate([[0], np.cumsum(lab_n)])[:-1]
    assert int(lab_n.sum()) == len(want) > 0
    first_pair = np.concatenate([[0], np.cumsum(lens)])[:-1]
    return gl, want, slot, lab_off, lab_n, first_pair


def test_the_numpy_assembly_equals_the_host_expansion(oracle):
    """The expected arena of the GPU test is put together with numpy indexing (the Python expansion is far too slow for
    a million pairs): at 2049 pairs it equals GlyphLabelList.to_label_list, arena and per-label ranges; and the
    triangle draws pixels."""
    table = labels.GlyphTable([[], TRIANGLE])
    gl, want, slot, lab_off, lab_n, _ = _case(table, 2049)
    ll = gl.to_label_list(table)
    assert np.array_equal(_bits(ll.segs), _bits(want))
    assert np.array_equal(ll.labels["n_segs"][slot], lab_n)
    assert np.array_equal(ll.labels["seg_off"][slot][lab_n > 0], lab_off[lab_n > 0])
    assert not ll.labels["n_segs"][np.setdiff1d(np.arange(len(ll.labels)), slot)].any()
    xy, tot = oracle.rasterizer_pixels(want[:3])
    assert len(xy) >= 2 and (tot > 0.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n_pairs", [1, 1023, 1024, 1025, 2047, 2049, 1024 * 1024 + 1025])
def test_arena_and_label_ranges_at_the_scan_edges(gpu_ctx, oracle, table, n_pairs):
    gl, want, slot, lab_off, lab_n, first_pair = _case(table, n_pairs)
    lab = gl.labels
    scene = gpu_ctx.upload(TileBuilder(zoom=17, scale=1, canvas=(240, 240, 240)).build())
    scene.set_glyph_labels(gl)
    got = scene.read_label_segs()
    assert got.shape == want.shape
    bad = (_bits(got) != _bits(want)).any(axis=1)
    assert not bad.any(), f"{int(bad.sum())} of {len(want)} calls differ from the host expansion, first at call {int(np.nonzero(bad)[0][0])}"
    # downstream: a label's n_segs / seg_off name its own calls
    gpu_ctx.render(scene)
    sample = {0, len(slot) - 1, len(slot) // 2}
    for edge in (1024, 2048, 1024 * 1024, 1024 * 1024 + 1024):
        k = int(np.searchsorted(first_pair, edge, side="right")) - 1
        sample |= {j for j in (k - 1, k, k + 1) if 0 <= j < len(slot)}
    drawn = 0
    for k in sorted(sample):
        segs = want[lab_off[k] : lab_off[k] + lab_n[k]]
        drawn += len(segs) > 0
        lc.check_plane(scene, oracle, int(slot[k]), segs, lc.TILE, f"label {int(slot[k])} (pairs from {int(first_pair[k])})")
    assert drawn >= 1
    for l in np.nonzero(lab["n_segs"] == 0)[0][:3]:
        assert scene.read_label_cover(int(l))[2].shape[0] == 0
    scene.free()
