"""Host pixels and PNG files from any scene (osmt_render_scene_host, osmt_render_scene_png, osmt_render_scene_png_begin,
osmt_render_scene_png_device, osmt_debug_png_offsets; k_png_offsets in osm_renderer_amd/csrc/osmt_pngenc.hip).

The yardsticks are not under test: the batch entries (osmt_render_batch_png / _host / _rgb), whose files and pixels the
scene forms must repeat byte for byte where both exist; the byte model of the encoder (tests/_png_model.py); the device's own
framebuffer (osmt_render_scene) for whole batches; the oracle for samples; numpy.cumsum in uint64 for the offset scan."""
import ctypes as C
import io
import subprocess
import threading

import numpy as np
import pytest

from osm_renderer_amd import abi, labels, lib, styled, synth
from osm_renderer_amd.lib import OsmtError
from tests import _anchors as an
from tests import _arealabels as al
from tests import _png_model, _scenepng
from tests import _text_placer_model as placer
from tests import _tilelabels as tl
from tests._styled_feed import geodata_of
from tests._tilequery import center_z18
from tests.test_gpu_area_labels import TX, TY, Z, _images, _latlon, _oracle_labels, tables, town  # noqa: F401  (tables, town: fixtures)

pytestmark = pytest.mark.gpu

CX, CY = center_z18()
GROUP = abi.PNG_OFFSETS_GROUP


def _decode(png):
    from PIL import Image

    return np.array(Image.open(io.BytesIO(png)).convert("RGB"))


def _tiles(n, scale=1, ops=4, x0=19000, y0=10000):
    return synth.make_tiles(synth.config_tiles(n, x0=x0, y0=y0), n_poly=ops, n_line=ops, scale=scale)


def _no_tiles():
    dl = synth.config2(1)
    dl.jobs, dl.ops = dl.jobs[:0], dl.ops[:0]
    return dl


def _three_comparisons(ctx, scene, files, ref=None):
    """every file equals the byte model of the device's framebuffer and decodes to it — and to the oracle's pixels, where given"""
    fb = ctx.render(scene).cpu().numpy()
    assert len(files) == scene.n_jobs == len(fb)
    for i, png in enumerate(files):
        assert png == _png_model.encode(fb[i]), f"tile {i}: bytes differ from the model"
        assert np.array_equal(_decode(png), fb[i][..., :3]), f"tile {i}: decoded pixels differ from the framebuffer"
        if ref is not None:
            assert np.array_equal(_decode(png), ref[i][..., :3]), f"tile {i}: decoded pixels differ from the oracle"
    return fb


def _host_forms_equal(ctx, scene, fb):
    assert np.array_equal(ctx.render_scene_host(scene), fb)
    assert np.array_equal(ctx.render_scene_host(scene, rgb=True).reshape(fb.shape[:3] + (3,)), fb[..., :3])


# ---- equal to the batch form -----------------------------------------------------------------------------------------------
def test_scene_forms_equal_the_batch_forms(gpu_ctx, oracle):
    dl = _tiles(5, ops=12)
    ll = labels.make_labels(5, labels_per_tile=6, seed=8)
    scene = gpu_ctx.upload(dl, ll)
    files = gpu_ctx.render_scene_png(scene)
    assert files == gpu_ctx.render_batch_png(dl, ll)
    want = oracle.render_batch(dl, threads=5, labels=ll)
    for i, png in enumerate(files):
        assert np.array_equal(_decode(png), want[i][..., :3])
    assert np.array_equal(gpu_ctx.render_scene_host(scene), gpu_ctx.render_batch_host(dl, ll))
    assert np.array_equal(gpu_ctx.render_scene_host(scene, rgb=True), gpu_ctx.render_batch_rgb(dl, ll))
    assert not np.array_equal(gpu_ctx.render_scene_host(scene), gpu_ctx.render_batch_host(dl))  # the labels are in the pixels
    assert gpu_ctx.render_scene_png(scene) == files  # borrowed: the same again
    scene.free()


# ---- label forms the batch PNG entry cannot take ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["glyphs", "text", "strings"])
def test_label_forms_the_batch_png_entry_cannot_take(gpu_ctx, oracle, form):
    syn = labels.synth_glyph_table()
    gpu_ctx.register_glyphs(syn)
    dl = _tiles(3, ops=8, x0=19020)
    kw = dict(labels_per_tile=8, seed=31, line_frac=0.4, empty_frac=0.05)
    scene = gpu_ctx.upload(dl)
    if form == "glyphs":
        gl = labels.make_glyph_labels(3, syn, **kw)
        scene.set_glyph_labels(gl)
        ll = gl.to_label_list(syn)
    elif form == "text":
        tx = labels.make_text_labels(3, syn, **kw)
        scene.set_text_labels(tx)
        ll = placer.place_text_labels(tx).to_label_list(syn)
    else:
        sl, font = labels.make_string_labels(3, syn, **kw)
        gpu_ctx.register_font(font)
        sl.with_font(font)
        scene.set_string_labels(sl)
        ll = placer.place_text_labels(sl.to_text_label_list(font)).to_label_list(syn)
    assert len(ll.segs) > 100
    files = gpu_ctx.render_scene_png(scene)
    fb = _three_comparisons(gpu_ctx, scene, files, oracle.render_batch(dl, threads=3, labels=ll))
    _host_forms_equal(gpu_ctx, scene, fb)
    bare = gpu_ctx.upload(dl)
    assert not np.array_equal(gpu_ctx.render(bare).cpu().numpy(), fb)  # the labels are in the pixels
    bare.free()
    scene.free()


# ---- built scenes -----------------------------------------------------------------------------------------------------------
def test_tile_built_scene_labelled_on_the_device(gpu_ctx, oracle, tables, town):  # noqa: F811
    W = town
    far = [(Z, TX + 500, TY + 500), (Z, TX + 501, TY + 500)]  # no index tile near: plain canvas, in the middle and at the end
    tiles = [(Z, TX, TY), (Z, TX + 1, TY), far[0], (Z, TX + 2, TY + 1), far[1]]
    sc = W.scene(tiles)
    got, _ = sc.build_tile_labels_all({Z: W.all[0]}, None)
    n = np.diff(got.job_label_off).tolist()
    assert n[2] == 0 and n[4] == 0 and min(n[0], n[1], n[3]) >= 6
    ref = oracle.render_batch(_latlon(sc.dl), images=_images(tables), threads=5, labels=_oracle_labels(got, tables))
    files = gpu_ctx.render_scene_png(sc)
    fb = _three_comparisons(gpu_ctx, sc, files, ref)
    assert len(np.unique(fb[2].reshape(-1, 4), axis=0)) == 1 and len(np.unique(fb[0].reshape(-1, 4), axis=0)) > 3
    _host_forms_equal(gpu_ctx, sc, fb)
    assert np.array_equal(gpu_ctx.render(sc).cpu().numpy(), fb)  # borrowed: the scene renders the same afterwards
    job = gpu_ctx.scene_png_begin(sc)
    assert gpu_ctx.png_end(job, np.empty(5 << 18, np.uint8), as_bytes=True) == files
    sc.free()


def test_styled_built_scene(gpu_ctx, oracle, tables, town):  # noqa: F811
    W = town
    st = np.zeros(2, styled.STYLE_REC_DTYPE)
    st["has_fill_color"], st["fill_color"], st["is_foreground_fill"] = 1, [(170, 200, 150), (90, 120, 200)], 1
    first = gpu_ctx.register_styles(st)
    tile = lambda i, j: (Z, TX + i, TY + j, [(3 * (10 * j + i) + 1, first), (3 * (10 * j + i) + 2, first + 1)], [(10 * j + i, first + 1)])
    tiles = [tile(0, 0), tile(4, 2), (Z, TX + 5, TY + 5, [], []), tile(9, 6), (Z, TX + 6, TY + 5, [], [])]
    sc = gpu_ctx.build_styled(styled.StyledBatch(W.gid, tiles))
    ref = oracle.render_batch(_latlon(sc.dl), threads=5)
    files = gpu_ctx.render_scene_png(sc)
    fb = _three_comparisons(gpu_ctx, sc, files, ref)
    assert len(np.unique(fb[2].reshape(-1, 4), axis=0)) == 1 and len(np.unique(fb[1].reshape(-1, 4), axis=0)) >= 3
    _host_forms_equal(gpu_ctx, sc, fb)
    assert np.array_equal(gpu_ctx.render(sc).cpu().numpy(), fb)
    sc.free()


# ---- chunk edges of the PNG pipeline ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, scale", [(1023, 1), (1024, 1), (1025, 1), (255, 2), (256, 2), (257, 2)])
def test_chunk_edges_of_the_png_pipeline(gpu_ctx, n, scale):
    """the job splits in two chunks from n >= 2 * (512 / scale^2) tiles on"""
    min_chunk = 512 // (scale * scale)
    chunk = n if n < 2 * min_chunk else max(min_chunk, (n + 1) // 2)
    assert (chunk == n) == (n in (1023, 255))
    scene = gpu_ctx.upload(_tiles(n, scale=scale, ops=2))
    fb = gpu_ctx.render(scene)
    slots, lens = gpu_ctx.encode_png_device(fb)
    slots, lens = slots.cpu().numpy(), lens.cpu().numpy().astype(np.int64)
    out, off = gpu_ctx.render_scene_png(scene, as_bytes=False)
    off = off.astype(np.int64)
    assert off[0] == 0 and np.array_equal(np.diff(off), lens)
    for i in range(n):
        assert np.array_equal(out[off[i] : off[i + 1]], slots[i, : lens[i]]), f"file {i}"
    edges = sorted({e for first in range(0, n, chunk) for e in (first, min(first + chunk, n) - 1)})
    assert len(edges) == (2 if chunk == n else 4)
    for i in edges:
        assert out[off[i] : off[i + 1]].tobytes() == _png_model.encode(fb[i].cpu().numpy()), f"file {i}: bytes differ from the model"
    scene.free()


# ---- routes of osmt_render_scene_host ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, pinned", [(1, True), (16, True), (17, True), (1, False), (16, False), (17, False), (255, True), (256, True), (257, True)])
def test_routes_of_render_scene_host(gpu_ctx, n, pinned):
    """zero-copy up to OSMT_ZERO_COPY_TILES = 16 tiles into pinned memory, the chunked read-back from 2 * 128 tiles on into
    pinned memory, one copy otherwise; tight and padded strides, RGBA8 and RGB8"""
    scene = gpu_ctx.upload(_tiles(n, ops=3, x0=19040))
    want = gpu_ctx.render(scene).cpu().numpy()
    px = 256 * 256
    for rgb, stride in ((False, 4 * px), (False, 4 * px + 64), (True, 3 * px), (True, 3 * px + 8)):
        out = gpu_ctx.host_alloc((n, stride)) if pinned else np.empty((n, stride), np.uint8)
        out[:] = 0x5A
        got = gpu_ctx.render_scene_host(scene, rgb=rgb, out=out, stride=stride)
        assert got is out
        ch = 3 if rgb else 4
        assert np.array_equal(out[:, : ch * px].reshape(n, 256, 256, ch), want[..., :ch]), (rgb, stride)
        assert (out[:, ch * px :] == 0x5A).all()  # the padding is the caller's
        if pinned:
            gpu_ctx.host_free(out)
    scene.free()


# ---- begin / end ------------------------------------------------------------------------------------------------------------
def test_begin_end_on_scenes(gpu_ctx):
    a, b = gpu_ctx.upload(_tiles(7, x0=19060)), gpu_ctx.upload(_tiles(3, x0=19080), labels.make_labels(3, labels_per_tile=4, seed=5))
    want_a, want_b = gpu_ctx.render_scene_png(a), gpu_ctx.render_scene_png(b)
    buf = lambda: np.empty(8 << 18, np.uint8)
    # two scenes in flight from one thread
    ja, jb = gpu_ctx.scene_png_begin(a), gpu_ctx.scene_png_begin(b)
    assert gpu_ctx.png_end(ja, buf(), as_bytes=True) == want_a and gpu_ctx.png_end(jb, buf(), as_bytes=True) == want_b
    # two jobs on the SAME scene, begun back to back: serialised, both complete
    j1, j2 = gpu_ctx.scene_png_begin(a), gpu_ctx.scene_png_begin(a)
    assert gpu_ctx.png_end(j2, buf(), as_bytes=True) == want_a and gpu_ctx.png_end(j1, buf(), as_bytes=True) == want_a
    # a too small buffer: the size needed is reported, the job is released, the scene is not
    job = gpu_ctx.scene_png_begin(a)
    with pytest.raises(OsmtError) as e:
        gpu_ctx.png_end(job, np.empty(100, np.uint8))
    total = sum(len(f) for f in want_a)
    assert e.value.code == abi.INVALID_ARG and "out_capacity" in str(e.value) and str(total) in str(e.value)
    assert job.offsets.tolist() == np.concatenate([[0], np.cumsum([len(f) for f in want_a])]).tolist()
    with pytest.raises(RuntimeError):
        gpu_ctx.png_end(job, buf())  # ended once
    assert gpu_ctx.render_scene_png(a) == want_a
    # a job dropped unended
    job = gpu_ctx.scene_png_begin(b)
    del job
    assert gpu_ctx.render_scene_png(b) == want_b
    fb = gpu_ctx.render(b).cpu().numpy()
    assert [_png_model.encode(t) for t in fb] == want_b
    # mixed with the batch form's jobs
    dl = _tiles(2, x0=19090)
    jd, ja = gpu_ctx.png_begin(dl), gpu_ctx.scene_png_begin(a)
    assert gpu_ctx.png_end(jd, buf(), as_bytes=True) == gpu_ctx.render_batch_png(dl) and gpu_ctx.png_end(ja, buf(), as_bytes=True) == want_a
    a.free()
    b.free()


def test_eight_threads_each_with_its_own_scene(gpu_ctx):
    lists = [_tiles(2 + k % 3, x0=19100 + 7 * k, y0=10010 + k) for k in range(8)]
    want = [gpu_ctx.render_batch_png(dl) for dl in lists]
    got, errors = [None] * 8, []

    def work(k):
        try:
            scene = gpu_ctx.upload(lists[k])
            first = gpu_ctx.render_scene_png(scene)
            px = gpu_ctx.render_scene_host(scene, rgb=True)
            job = gpu_ctx.scene_png_begin(scene)
            second = gpu_ctx.png_end(job, np.empty(4 << 18, np.uint8), as_bytes=True)
            scene.free()
            got[k] = (first, second, px)
        except Exception as e:  # reported by the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(8):
        assert got[k][0] == want[k] and got[k][1] == want[k], f"thread {k}"
        for i, png in enumerate(want[k]):
            assert np.array_equal(_decode(png).reshape(-1), got[k][2][i]), f"thread {k} tile {i}"


# ---- the device form --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 64, 65])
def test_device_form(gpu_ctx, n):
    import torch

    scene = gpu_ctx.upload(_tiles(n, x0=19200) if n else _no_tiles())
    assert scene.n_jobs == n
    host = gpu_ctx.render_scene_png(scene)
    sizes = [len(f) for f in host]
    want_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    total = int(want_off[-1])
    need = lib.load().osmt_scene_png_work_bytes(gpu_ctx._h, scene._h)
    assert need == renderer_layout(n)[3]
    # capacity exactly the total
    png = torch.full((total,), 0xC3, dtype=torch.uint8, device=gpu_ctx.device)
    _, off, status = gpu_ctx.render_scene_png_device(scene, png=png)
    assert status.cpu().tolist() == [0]
    assert np.array_equal(off.cpu().numpy().view(np.uint64), want_off)
    assert png.cpu().numpy().tobytes() == b"".join(host)
    if n:  # one byte less: nothing is written, the offsets are complete
        small = torch.full((total - 1,), 0x5A, dtype=torch.uint8, device=gpu_ctx.device)
        _, off, status = gpu_ctx.render_scene_png_device(scene, png=small)
        assert status.cpu().tolist() == [1]
        assert np.array_equal(off.cpu().numpy().view(np.uint64), want_off)
        assert (small == 0x5A).all().item()
    assert gpu_ctx.render_scene_png(scene) == host  # and the scene is as it was
    scene.free()


def renderer_layout(n, dim=256):
    from osm_renderer_amd import renderer

    return renderer.scene_png_work_layout(n, dim)


# ---- the scan alone ---------------------------------------------------------------------------------------------------------
def _scan(ctx, lengths, capacity):
    import torch

    lengths = np.asarray(lengths, dtype=np.uint32)
    t = torch.from_numpy(lengths.view(np.int32).copy()).to(ctx.device)
    off, status = ctx.debug_png_offsets(t, capacity)
    return off.cpu().numpy().view(np.uint64), int(status.cpu()[0])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP + 1])
def test_offset_scan_against_cumsum(gpu_ctx, n):
    rng = np.random.default_rng(1000 + n)
    for kind in ("file sizes", "any 32 bits", "zeros"):
        hi = {"file sizes": 300_000, "any 32 bits": 1 << 32, "zeros": 1}[kind]
        lengths = rng.integers(0, hi, size=n, dtype=np.uint64).astype(np.uint32)
        want = np.concatenate([[0], np.cumsum(lengths.astype(np.uint64), dtype=np.uint64)]).astype(np.uint64)
        total = int(want[-1])
        for capacity, flag in ((total, 0), (total + 1, 0), ((1 << 64) - 1, 0)) + (((total - 1, 1),) if total else ()):
            got, status = _scan(gpu_ctx, lengths, capacity)
            assert got.shape == want.shape and np.array_equal(got, want), (kind, np.nonzero(got != want)[0][:4])
            assert status == flag, (kind, capacity, total)


def test_offset_scan_carries_past_32_bits(gpu_ctx):
    big = 0xFFFFFFFF
    got, status = _scan(gpu_ctx, [big, big], 2 * big)
    assert got.tolist() == [0, big, 2 * big] and status == 0 and 2 * big > 1 << 32
    assert _scan(gpu_ctx, [big, big], 2 * big - 1)[1] == 1
    assert _scan(gpu_ctx, [big, big], (1 << 32) - 1)[1] == 1  # a comparison in 32 bits would let 2 * big = 0x1FFFFFFFE through as 0xFFFFFFFE
    # the carry from pass to pass and from wave to wave: every length the largest, over three passes and a bit
    lengths = np.full(3 * GROUP + 5, big, np.uint32)
    got, status = _scan(gpu_ctx, lengths, 0)
    assert np.array_equal(got, np.arange(len(lengths) + 1, dtype=np.uint64) * np.uint64(big)) and status == 1


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_each_followed_by_a_correct_call(gpu_ctx):
    import torch

    from osm_renderer_amd.renderer import Context

    L, h = lib.load(), gpu_ctx._h
    scene = gpu_ctx.upload(_tiles(2, x0=19300))
    want = gpu_ctx.render(scene).cpu().numpy()
    files = gpu_ctx.render_scene_png(scene)
    px = 256 * 256
    out = np.zeros(2 * 4 * px + 64, np.uint8)
    out = out[(-out.ctypes.data) % 4 :]  # 4-byte aligned
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    off = (C.c_uint64 * 3)()

    def good():
        assert np.array_equal(gpu_ctx.render_scene_host(scene), want) and gpu_ctx.render_scene_png(scene) == files

    def refused(rc, *words):
        msg = L.osmt_last_error().decode()
        assert rc == abi.INVALID_ARG and all(w in msg for w in words), (rc, msg)
        good()

    refused(L.osmt_render_scene_host(None, scene._h, 0, ptr(out), 4 * px), "NULL")
    refused(L.osmt_render_scene_host(h, None, 0, ptr(out), 4 * px), "NULL")
    refused(L.osmt_render_scene_host(h, scene._h, 0, None, 4 * px), "NULL")
    refused(L.osmt_render_scene_host(h, scene._h, 2, ptr(out), 4 * px), "unknown pixel format 2")
    refused(L.osmt_render_scene_host(h, scene._h, 0, ptr(out), 4 * px - 1), "out_tile_stride_bytes < W*H*4")
    refused(L.osmt_render_scene_host(h, scene._h, 1, ptr(out), 3 * px - 1), "out_tile_stride_bytes < W*H*3")
    refused(L.osmt_render_scene_host(h, scene._h, 1, ptr(out), 3 * px + 2), "not a multiple of 4")
    refused(L.osmt_render_scene_host(h, scene._h, 1, ptr(out[1:]), 3 * px), "not a multiple of 4")
    assert L.osmt_render_scene_host(h, scene._h, 0, ptr(out[1:]), 4 * px + 3) == abi.OK  # RGBA8 asks for neither
    assert np.array_equal(np.stack([out[1 + i * (4 * px + 3) :][: 4 * px] for i in range(2)]).reshape(want.shape), want)
    refused(L.osmt_render_scene_png(h, scene._h, ptr(out), out.size, None), "NULL")
    refused(L.osmt_render_scene_png(h, scene._h, None, 10, off), "NULL")
    refused(L.osmt_render_scene_png(h, None, ptr(out), out.size, off), "NULL")
    job = C.c_void_p(5)
    refused(L.osmt_render_scene_png_begin(h, None, C.byref(job)), "NULL")
    assert job.value is None
    refused(L.osmt_render_scene_png_begin(h, scene._h, None), "NULL")
    # capacity too small: the one-piece call reports the size needed, as the batch form does
    assert L.osmt_render_scene_png(h, scene._h, ptr(out), 10, off) == abi.INVALID_ARG
    assert "out_capacity" in L.osmt_last_error().decode() and list(off) == [0, len(files[0]), len(files[0]) + len(files[1])]
    good()
    # a scene of another context
    other = Context(0)
    theirs = other.upload(_tiles(2, x0=19300))
    refused(L.osmt_render_scene_host(h, theirs._h, 0, ptr(out), 4 * px), "another context")
    refused(L.osmt_render_scene_png(h, theirs._h, ptr(out), out.size, off), "another context")
    refused(L.osmt_render_scene_png_begin(h, theirs._h, C.byref(job)), "another context")
    assert L.osmt_scene_png_work_bytes(h, theirs._h) == 0 and L.osmt_scene_png_work_bytes(h, scene._h) > 0
    dev = torch.zeros(64, dtype=torch.uint8, device=gpu_ctx.device)
    d = lambda k: C.c_void_p(dev.data_ptr() + k)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    refused(L.osmt_render_scene_png_device(h, theirs._h, d(0), 64, d(0), 0, d(0), d(32), st), "another context")
    assert other.render_scene_png(theirs) == files  # the same tiles: the same files from the context that owns the scene
    theirs.free()
    other.close()
    # the device form's own: a work buffer that is too small or not aligned
    need = L.osmt_scene_png_work_bytes(h, scene._h)
    work = torch.empty(need + 256, dtype=torch.uint8, device=gpu_ctx.device)
    w = lambda k: C.c_void_p(work.data_ptr() + k)
    refused(L.osmt_render_scene_png_device(h, scene._h, w(0), need - 1, d(0), 0, d(0), d(32), st), "work_bytes")
    refused(L.osmt_render_scene_png_device(h, scene._h, w(4), need, d(0), 0, d(0), d(32), st), "aligned")
    refused(L.osmt_render_scene_png_device(h, scene._h, None, need, d(0), 0, d(0), d(32), st), "NULL")
    refused(L.osmt_render_scene_png_device(h, scene._h, w(0), need, None, 8, d(0), d(32), st), "NULL")
    assert L.osmt_render_scene_png_device(h, scene._h, w(0), need, None, 0, d(0), d(32), st) == abi.OK  # no blob: sizes only
    torch.cuda.synchronize()
    got = dev.cpu().numpy()
    assert got[:24].view(np.uint64).tolist() == [0, len(files[0]), len(files[0]) + len(files[1])] and got[32:36].view(np.uint32)[0] == 1
    # a scene of 0 tiles is valid everywhere
    empty = gpu_ctx.upload(_no_tiles())
    assert gpu_ctx.render_scene_png(empty) == [] and gpu_ctx.render_scene_host(empty).shape == (0, 256, 256, 4)
    off[0] = 7
    assert L.osmt_render_scene_png(h, empty._h, None, 0, off) == abi.OK and off[0] == 0
    job = gpu_ctx.scene_png_begin(empty)
    _, o = gpu_ctx.png_end(job, np.empty(1, np.uint8))
    assert o.tolist() == [0]
    empty.free()
    good()
    scene.free()


# ---- the C++ binding --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1, 2])
def test_cpp_demo_files_decode_to_the_python_paths_pixels(gpu_ctx, tmp_path, scale):
    """tests/scene_png_host_demo.cpp (Context::render_tiles_png, TileScene::render_png / render_host) in a process of its own;
    the same world, styles and bindings registered here give the pixels its files must decode to"""
    w = al.World((CX, CY))
    rect = lambda x, y, a, b: [(x, y), (x + a, y), (x + a, y + b), (x, y + b), (x, y)]
    near, east = (CX, CY), (CX + 1, CY)
    w.way(w.shape(rect(20, 20, 60, 60)), 5, [near])
    w.way(w.shape(rect(120, 40, 50, 70)), 6, [near])
    w.way(w.shape(rect(30, 150, 80, 40)), 7, [near])
    w.way(w.shape(rect(150, 150, 60, 60), east), 8, [east])
    w.mp([w.polygon(w.shape(rect(100, 100, 30, 30)))], 9, [near])
    path = tmp_path / "w.bin"
    r, refs = w.write(path)
    tiles = [(18, CX, CY), (18, CX + 9, CY + 9), (18, CX + 1, CY), (17, CX >> 1, CY >> 1)]
    out = subprocess.run([_scenepng.build_demo(), str(path), str(scale), str(tmp_path)] + [str(v) for t in tiles for v in t],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr[-2000:])
    word, n_files, n_bytes = out.stdout.split()
    files = [(tmp_path / f"tile_{i}.png").read_bytes() for i in range(len(tiles))]
    assert word == "OK" and int(n_files) == len(tiles) and int(n_bytes) == sum(len(f) for f in files)
    # the Python path
    g = geodata_of(r)
    gid = gpu_ctx.register_geodata(g)
    gpu_ctx.register_tile_index(gid, styled.TileIndex([(k, refs[k][1], refs[k][2]) for k in sorted(refs)]))
    f = an.mercator_factors(r.node_table())
    gpu_ctx.register_node_mercator(gid, f)
    st = np.zeros(1, styled.STYLE_REC_DTYPE)
    st["has_fill_color"], st["fill_color"], st["is_foreground_fill"] = 1, (170, 200, 150), 1
    draw = gpu_ctx.register_styles(st)
    bind = gpu_ctx.register_style_bindings(styled.StyleBindings(gid, 0, 18, [[draw]] * r.n_ways, [[draw]] * r.n_multipolygons))
    icon = ((37 * np.arange(7 * 3 * 4) + 11) % 256).astype(np.uint8).reshape(7, 3, 4)
    icon[..., 3] = 255
    ls = gpu_ctx.register_label_styles(tl.label_styles([dict(icon=gpu_ctx.register_image(icon))]))
    lb = gpu_ctx.register_area_label_bindings(styled.AreaLabelBindings(gid, 0, 18, [[(ls, None)] if i % 2 else [] for i in range(r.n_ways)],
                                                                       [[(ls, None)]] * r.n_multipolygons))
    sc = gpu_ctx.build_tiles(styled.TileBatch(gid, tiles, {z: bind for z in range(19)}, scale=scale, canvas=(241, 238, 232)))
    area, _ = sc.build_tile_labels_all({z: lb for z in range(19)}, None)
    assert (area.labels["has_icon"] == 1).sum() >= 4
    want = gpu_ctx.render(sc).cpu().numpy()
    assert gpu_ctx.render_scene_png(sc) == files
    rgb = np.frombuffer((tmp_path / "tiles.rgb").read_bytes(), np.uint8).reshape(want.shape[:3] + (3,))
    for i, png in enumerate(files):
        assert np.array_equal(_decode(png), want[i][..., :3]) and np.array_equal(rgb[i], want[i][..., :3]), f"tile {i}"
    assert len(np.unique(want[0].reshape(-1, 4), axis=0)) > 3 and len(np.unique(want[1].reshape(-1, 4), axis=0)) == 1
    sc.free()
    r.close()
