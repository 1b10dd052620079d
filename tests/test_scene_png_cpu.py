"""Host pixels and PNG files from a scene (osmt_render_scene_host, osmt_render_scene_png[_begin], osmt_render_scene_png_device,
osmt_debug_png_offsets): what needs no device — the NULL-argument refusals, which come before the first HIP call, and the
documented layout of the device form's work buffer against a restatement of its arithmetic."""
import ctypes as C

import pytest

from osm_renderer_amd import abi, lib, renderer

ONE = C.c_void_p(256)  # a non-NULL, aligned stand-in: every call below is refused before anything is dereferenced


def _refused(rc, *words):
    msg = lib.load().osmt_last_error().decode()
    assert rc == abi.INVALID_ARG and all(w in msg for w in words), (rc, msg)


def test_null_arguments_are_refused_without_a_device():
    L = lib.load()
    off, job = (C.c_uint64 * 2)(), C.c_void_p(77)
    for ctx, scene, out in ((None, ONE, ONE), (ONE, None, ONE), (ONE, ONE, None)):
        _refused(L.osmt_render_scene_host(ctx, scene, abi.PIXELS_RGBA8, out, 1 << 20), "NULL argument")
    for ctx, scene, png, cap, o in ((None, ONE, ONE, 16, off), (ONE, None, ONE, 16, off), (ONE, ONE, ONE, 16, None), (ONE, ONE, None, 16, off)):
        _refused(L.osmt_render_scene_png(ctx, scene, png, cap, o), "NULL argument")
    for ctx, scene, pj in ((None, ONE, C.byref(job)), (ONE, None, C.byref(job)), (ONE, ONE, None)):
        job.value = 77
        _refused(L.osmt_render_scene_png_begin(ctx, scene, pj), "NULL argument")
        assert pj is None or job.value is None  # *out_job is cleared whenever there is one
    for ctx, scene, d_off, d_status in ((None, ONE, ONE, ONE), (ONE, None, ONE, ONE), (ONE, ONE, None, ONE), (ONE, ONE, ONE, None)):
        _refused(L.osmt_render_scene_png_device(ctx, scene, ONE, 1 << 30, ONE, 1 << 30, d_off, d_status, None), "NULL argument")
    for ctx, d_len, n, d_off, d_status in ((None, ONE, 4, ONE, ONE), (ONE, None, 4, ONE, ONE), (ONE, ONE, 4, None, ONE), (ONE, ONE, 4, ONE, None),
                                           (None, None, 0, ONE, ONE)):
        _refused(L.osmt_debug_png_offsets(ctx, d_len, n, 0, d_off, d_status, None), "NULL argument")
    _refused(L.osmt_render_batch_png_end(None, None, 0, off), "NULL job")  # the shared second half, as before


def test_work_bytes_of_bad_arguments_is_zero():
    L = lib.load()
    assert L.osmt_scene_png_work_bytes(None, None) == 0
    assert L.osmt_scene_png_work_bytes(ONE, None) == 0 and L.osmt_scene_png_work_bytes(None, ONE) == 0


@pytest.mark.parametrize("scale", [1, 2, 3, 4])
def test_work_layout_is_the_documented_one(scale):
    """include/osmtile.h: n framebuffers of W*W*4 bytes, then n slots of osmt_png_device_bound(W, W) bytes, then n 32-bit
    lengths, each part rounded up to a multiple of 256 bytes; 0 tiles: 0 bytes."""
    L = lib.load()
    W = abi.TILE_SIZE * scale
    slot = L.osmt_png_device_bound(W, W)
    assert slot % 4 == 0 and slot > W * (3 * W + 1)
    for n in (0, 1, 3, 63, 64, 65, 1025):
        parts = [n * W * W * 4, n * slot, n * 4]
        want, at = [], 0
        for p in parts:
            want.append(at)
            at += -(-p // 256) * 256
        got = renderer.scene_png_work_layout(n, W)
        assert list(got) == want + [at], (n, got)
        assert all(v % 256 == 0 for v in got) and (n > 0 or got[3] == 0)
        if n:  # the parts do not overlap and the lengths' part ends inside the buffer
            assert got[1] >= parts[0] and got[2] - got[1] >= parts[1] and got[3] - got[2] >= parts[2]
