"""The glyph-run path of the C++ host mirror (Rasterizer::draw_glyph -> TilePixels -> osmt_render_batch_rgb_glyphs)
against the same labels drawn with the reference's glyph walk on the host (draw_line / draw_quad): identical tiles."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_mirror_glyph_demo.cpp")
BIN = os.path.join(ROOT, "tests", "_build", "host_mirror_glyph_demo")


def build_glyph_demo():
    hdr = os.path.join(ROOT, "osm_renderer_amd", "host", "osmt_draw.hpp")
    libdir = os.path.join(ROOT, "osm_renderer_amd")
    lib = os.path.join(libdir, "libosmtile.so")
    assert os.path.exists(lib), "build libosmtile.so first (__graft_entry__.build())"
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(SRC), os.path.getmtime(hdr), os.path.getmtime(lib)):
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        tmp = f"{BIN}.{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", tmp, SRC, "-L" + libdir, "-losmtile",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
        os.replace(tmp, BIN)
    return BIN


def test_host_mirror_glyph_demo_builds():
    """CPU-side: the glyph-run recorder of the mirror compiles and links against the C ABI."""
    assert os.path.exists(build_glyph_demo())


@pytest.mark.gpu
def test_host_mirror_glyph_runs_equal_the_host_glyph_walk(gpu_ctx, tmp_path):
    import torch

    out = tmp_path / "glyphs.rgb"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([build_glyph_demo(), str(out)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"demo exit {r.returncode}: {r.stderr}"  # 4 / 5: TileBatch took a glyph-run tile
    runs, calls, plain = np.fromfile(out, dtype=np.uint8).reshape(3, 256, 256, 3)
    np.testing.assert_array_equal(runs, calls)
    assert (runs != plain).any(-1).sum() > 100  # the labels drew something
