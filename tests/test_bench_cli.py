"""bench.py's launcher contract, the part that needs no GPU: `--gpus N` with fewer than N visible
devices must refuse to run (never a silent N = 1 run under an N-GPU label), whether or not a launcher set WORLD_SIZE.
Also what a plain run prints and what --dump-outputs writes."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES",
              "CUDA_VISIBLE_DEVICES"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=env,
                          timeout=300)


def _visible_gpus():
    import torch

    return torch.cuda.device_count()


def test_more_gpus_than_visible_is_refused():
    n = _visible_gpus() + 1
    r = _run(["--gpus", str(n), "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0
    assert "refusing to run" in (r.stderr + r.stdout)
    assert '"metric"' not in r.stdout  # no bench line under a wrong label


def test_refused_under_a_launcher_too():
    n = _visible_gpus() + 1
    r = _run(["--gpus", str(n), "--steps", "1", "--warmup", "0"],
             {"RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": str(n), "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29533"})
    assert r.returncode != 0
    assert "refusing to run" in (r.stderr + r.stdout)


def test_zero_gpus_is_an_error():
    r = _run(["--gpus", "0"])
    assert r.returncode != 0


def test_pinned_rank_without_a_device_is_refused():
    """A launcher that pins one device per rank (each rank sees 1 device of an N-GPU job) is trusted up to the rank count the
    path's all-reduce returns; a rank that sees NO device still refuses at once."""
    if _visible_gpus() != 0:
        import pytest

        pytest.skip("needs a host without GPUs")
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"],
             {"RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "2", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29534", "HIP_VISIBLE_DEVICES": "0"})
    assert r.returncode != 0
    assert "refusing to run" in (r.stderr + r.stdout)


def _dumped(d):
    import numpy as np

    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


def test_dump_outputs_is_float_exact_and_bounded(tmp_path):
    """--dump-outputs on a stand-in framebuffer batch: float32 / float64 arrays only, under 64 MB in all, the same seeded sample
    every time, and values equal to the RGBA8 bytes they were taken from."""
    import importlib.util

    import numpy as np
    import torch

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    fb = torch.randint(0, 256, (1024, 256, 256, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    bench.dump_outputs(fb, str(tmp_path / "a"))
    bench.dump_outputs(fb, str(tmp_path / "b"))
    a, b = _dumped(tmp_path / "a"), _dumped(tmp_path / "b")
    assert set(a) == {"tile_channel_sums", "framebuffer_sample", "framebuffer_sample_tiles"}
    assert all(a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]) for k in a)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 * 1000 * 1000
    fbn = fb.numpy()
    idx = a["framebuffer_sample_tiles"].astype(np.int64)
    assert len(idx) > 1 and np.array_equal(a["framebuffer_sample"], fbn[idx].astype(np.float32))
    assert np.array_equal(a["tile_channel_sums"], fbn.reshape(1024, -1, 4).astype(np.float64).sum(axis=1))


@pytest.mark.gpu
def test_plain_run_times_the_headline_only_and_dumps(tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` prints the headline (value, ms_per_step over exactly K steps) and none of
    the --full objects; --dump-outputs writes the last step's framebuffers."""
    import json

    r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "out")])
    assert r.returncode == 0, r.stderr[-600:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line
    assert line["steps"] == 3 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(line["config"]["tiles_per_step_all_gpus"] / line["ms_per_step"] * 1e3)
    assert not {"one_batch_at_a_time", "roofline", "config4_strong", "cpu_baseline", "sustained"} & set(line)
    out = _dumped(tmp_path / "out")
    assert out["tile_channel_sums"].shape == (1024, 4) and out["framebuffer_sample"].shape[1:] == (256, 256, 4)
    assert out["tile_channel_sums"][:, 3].min() > 0  # every tile was rendered: opaque canvas under everything
