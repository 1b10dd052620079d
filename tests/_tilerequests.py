"""Compiles tests/tile_server_host_demo.cpp (TileServer::render_png and Worker::render_tile_png of host/osmt_draw.hpp: tile
coordinates in, PNG files out) against libosmtile.so."""
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "_build", "tile_server_host_demo")


def build_demo():
    src = os.path.join(ROOT, "tests", "tile_server_host_demo.cpp")
    libdir = os.path.join(ROOT, "osm_renderer_amd")
    lib = os.path.join(libdir, "libosmtile.so")
    assert os.path.exists(lib), "build libosmtile.so first (__graft_entry__.build())"
    deps = [src, lib, os.path.join(ROOT, "include", "osmtile.h")] + glob.glob(os.path.join(libdir, "host", "*.hpp"))
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        tmp = f"{BIN}.{os.getpid()}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-pthread", "-o", tmp, src, "-L" + libdir, "-losmtile",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
        os.replace(tmp, BIN)
    return BIN
