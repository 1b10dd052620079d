"""k_png_encode_fast and k_png_encode (csrc/osmt_pngenc.hip) at their matcher, band and size edges: the case corpus of
tests/_png_cases.py — what each case is for, and that the model reaches it, is tests/test_png_cases_cpu.py — byte for byte against
tests/_png_model.py; alpha, dirty slots, a guard behind the last slot, strides and a stream of the caller's; OSMT_PNG_LZ=0
against the model without matches; and the shapes the entry refuses."""
import ctypes as C_
import hashlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from osm_renderer_amd import abi
from osm_renderer_amd.lib import OsmtError, load
from tests import _png_cases as C
from tests import _png_model as M

pytestmark = pytest.mark.gpu

SHAPES = list(C.by_shape())
_IDS = ["%dx%d" % s for s in SHAPES]
GUARD = 4096


def _decode(png):
    from PIL import Image

    return np.array(Image.open(io.BytesIO(png)).convert("RGB"))


def _files(gpu_ctx, imgs):
    import torch

    slots, lens = gpu_ctx.encode_png_device(torch.from_numpy(np.ascontiguousarray(imgs)).cuda())
    slots, lens = slots.cpu().numpy(), lens.cpu().numpy()
    return [slots[i, : lens[i]].tobytes() for i in range(len(imgs))], lens


def _check(cases, files, lens, what=""):
    for c, png, n in zip(cases, files, lens):
        want = C.model_file(c)
        assert int(n) == len(want), "%s%r: length %d, the model's file has %d bytes" % (what, c, n, len(want))
        assert png == want, "%s%r: bytes differ from the model" % (what, c)
        assert np.array_equal(_decode(png), c.img[..., :3]), "%s%r: decoded pixels differ" % (what, c)


@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_every_case_byte_for_byte(gpu_ctx, shape):
    """all cases of one shape in one call: different tiles share a launch"""
    cases = C.by_shape()[shape]
    files, lens = _files(gpu_ctx, np.stack([c.img for c in cases]))
    _check(cases, files, lens)


@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_alpha_is_ignored(gpu_ctx, shape):
    cases = C.by_shape()[shape]
    imgs = np.stack([c.img for c in cases])
    imgs[..., 3] = np.random.default_rng(shape[0] * 7 + shape[1]).integers(0, 256, size=imgs.shape[:3])
    files, lens = _files(gpu_ctx, imgs)
    _check(cases, files, lens, "random alpha, ")


def _encode_raw(gpu_ctx, cases, fill, tile_extra=0, png_extra=0, stream=None):
    """the C entry on buffers of the test's own: slots pre-filled with `fill`, GUARD bytes of `fill` behind the last slot.
    Returns (files, the guard as it is afterwards)."""
    import torch

    H, W = cases[0].shape
    n = len(cases)
    bound = load().osmt_png_device_bound(W, H)
    tile_stride, png_stride = H * W * 4 + tile_extra, bound + png_extra
    src = np.full((n, tile_stride), 0xA5, dtype=np.uint8)
    for i, c in enumerate(cases):
        src[i, : H * W * 4] = c.img.reshape(-1)
    d_src = torch.from_numpy(src).cuda()
    d_png = torch.full((n * png_stride + GUARD,), fill, dtype=torch.uint8, device="cuda")
    d_len = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream() if stream is None else stream
    s.wait_stream(torch.cuda.current_stream())
    rc = load().osmt_encode_png_device(gpu_ctx._h, C_.c_void_p(d_src.data_ptr()), tile_stride, n, W, H, C_.c_void_p(d_png.data_ptr()),
                                       png_stride, C_.c_void_p(d_len.data_ptr()), C_.c_void_p(s.cuda_stream))
    assert rc == abi.OK, load().osmt_last_error()
    s.synchronize()
    png, lens = d_png.cpu().numpy(), d_len.cpu().numpy()
    assert (lens > 0).all() and (lens <= bound).all()
    return [png[i * png_stride : i * png_stride + lens[i]].tobytes() for i in range(n)], lens, png[n * png_stride :]


def _worst_last(shape):
    cases = list(C.by_shape()[shape])
    cases.sort(key=lambda c: c.kind == "worst")  # (stable) a tile at the bit cap in the last slot, in front of the guard
    return cases


@pytest.mark.parametrize("shape", [(8, 256), (16, 512), (4, 1024), (16, 256), (1, 4)], ids=lambda s: "%dx%d" % s)
def test_dirty_slots_and_a_guard_behind_the_last_slot(gpu_ctx, shape):
    """png_stride is exactly osmt_png_device_bound: whatever a tile writes past its slot lands in the next tile's slot or in the
    guard.  The files do not depend on what the slots held before; the guard is untouched."""
    cases = _worst_last(shape)
    for fill in (0x00, 0xFF, 0xA5):
        files, lens, guard = _encode_raw(gpu_ctx, cases, fill)
        assert (guard == fill).all(), "fill %#x: %d guard bytes written" % (fill, int((guard != fill).sum()))
        _check(cases, files, lens, "fill %#x, " % fill)


@pytest.mark.parametrize("shape", [(8, 256), (16, 512), (4, 1024)], ids=lambda s: "%dx%d" % s)
def test_a_batch_of_two_tiles_at_the_bit_cap(gpu_ctx, shape):
    """two tiles, every filtered byte an lmax-bit literal, slots back to back: neither reaches into the other or into the guard"""
    cases = [c for c in C.by_shape()[shape] if c.kind == "worst"]
    assert len(cases) == 2
    files, lens, guard = _encode_raw(gpu_ctx, cases, 0xA5)
    assert (guard == 0xA5).all()
    _check(cases, files, lens)
    H, W = shape
    assert all(len(f) * 8 > H * (M.LITLEN[4] + 3 * W * M.LMAX) for f in files)


@pytest.mark.parametrize("shape", [(8, 256), (64, 512), (9, 1020)], ids=lambda s: "%dx%d" % s)
def test_strides_above_the_minimum_on_a_stream_of_the_callers(gpu_ctx, shape):
    """tile_stride = W * H * 4 + 16, png_stride = bound + 256 (multiples of 16: the fast path loads 16 bytes at a time), an
    explicit non-default stream"""
    import torch

    cases = _worst_last(shape)
    files, lens, guard = _encode_raw(gpu_ctx, cases, 0xFF, tile_extra=16, png_extra=256, stream=torch.cuda.Stream())
    assert (guard == 0xFF).all()
    _check(cases, files, lens, "strides, ")


_LZ_SHAPES = [(8, 256), (16, 256), (72, 256), (8, 512), (64, 512)]


def test_png_lz_0_writes_the_models_files_without_matches(gpu_ctx):
    """OSMT_PNG_LZ is read once per process: a child encodes the fast-shape cases and prints one sha256 per file"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child = (
        "import hashlib, sys; sys.path.insert(0, %r)\n"
        "import numpy as np, torch\n"
        "from osm_renderer_amd.renderer import Context\n"
        "from tests import _png_cases as C\n"
        "ctx = Context(0)\n"
        "for shape in %r:\n"
        "    cases = C.by_shape()[shape]\n"
        "    slots, lens = ctx.encode_png_device(torch.from_numpy(np.stack([c.img for c in cases])).cuda())\n"
        "    slots, lens = slots.cpu().numpy(), lens.cpu().numpy()\n"
        "    for i, c in enumerate(cases):\n"
        "        print('sha', shape[0], shape[1], c.name, hashlib.sha256(slots[i, :lens[i]].tobytes()).hexdigest())\n"
        "ctx.close()\n" % (root, _LZ_SHAPES)
    )
    out = subprocess.run([sys.executable, "-c", child], env=dict(os.environ, OSMT_PNG_LZ="0"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = {tuple(l.split()[1:4]): l.split()[4] for l in out.stdout.splitlines() if l.startswith("sha ")}
    n_differ = 0
    for shape in _LZ_SHAPES:
        for c in C.by_shape()[shape]:
            want = C.model_file(c, lz=False)
            assert got[(str(shape[0]), str(shape[1]), c.name)] == hashlib.sha256(want).hexdigest(), "%r without matches" % c
            n_differ += want != C.model_file(c)
    assert n_differ >= 12  # the matcher cases are not the same files without their matches


@pytest.mark.parametrize("shape", [(1025, 4), (1032, 256), (2048, 256)], ids=lambda s: "%dx%d" % s)
def test_heights_above_1024_are_refused(gpu_ctx, shape):
    """k_png_encode keeps a word per row in LDS arrays of 1024: the entry returns OSMT_UNSUPPORTED before any launch"""
    import torch

    H, W = shape
    with pytest.raises(OsmtError) as e:
        gpu_ctx.encode_png_device(torch.zeros((1, H, W, 4), dtype=torch.uint8, device="cuda"))
    assert e.value.code == abi.UNSUPPORTED
    assert "height %d" % H in str(e.value)


def test_height_1024_is_accepted(gpu_ctx):
    """1024 x 4 (generic kernel; in the corpus too) and 1024 x 256 (fast path, 128 rows per band)"""
    for H, W in ((1024, 4), (1024, 256)):
        c = C.plain(H, W)
        files, lens = _files(gpu_ctx, c.img[None])
        want = M.encode(c.img)
        assert int(lens[0]) == len(want) and files[0] == want
        assert np.array_equal(_decode(files[0]), c.img[..., :3])
