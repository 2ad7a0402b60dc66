"""bench.py argument contract checks that need no GPU: it refuses to run with a world size other
than --gpus, and refuses --gpus N when fewer than N GPUs are visible (here: none)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, **env_over):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "ROUTEST_BENCH_SHARE_GPU"):
        env.pop(k, None)
    env.update(env_over)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args,
                          capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)


def test_world_size_mismatch_exits_2():
    r = _run(["--gpus", "4", "--steps", "1"], WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    assert r.returncode == 2 and "WORLD_SIZE=2" in r.stderr


def test_dump_outputs_writes_a_fixed_float32_sample(tmp_path, monkeypatch):
    """``--dump-outputs``: a small output is written whole, a large one as the same seeded rows
    every time, float32, never more rows than the cap."""
    import importlib.util

    import numpy as np
    import torch
    spec = importlib.util.spec_from_file_location("routest_bench_script", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b.DUMP_ROWS * 4 <= 32 << 20
    out = torch.arange(1000, dtype=torch.float32) * 0.5
    b.dump_outputs(str(tmp_path / "whole"), out, 0, 1)
    got = np.load(tmp_path / "whole" / "eta_minutes.npy")
    assert got.dtype == np.float32 and np.array_equal(got, out.numpy())
    monkeypatch.setattr(b, "DUMP_ROWS", 256)
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), out, 0, 1)
    sa, sb = (np.load(tmp_path / d / "eta_minutes.npy") for d in ("a", "b"))
    assert sa.dtype == np.float32 and sa.shape == (256,) and np.array_equal(sa, sb)
    assert np.all(np.diff(sa) >= 0) and np.isin(sa, out.numpy()).all()
    b.dump_outputs(str(tmp_path / "r1"), out, 1, 2)        # one file per rank, the cap shared
    assert np.load(tmp_path / "r1" / "eta_minutes_rank1.npy").shape == (128,)


def test_too_many_gpus_exits_2():
    import torch
    if torch.cuda.device_count() >= 8:
        return
    r = _run(["--gpus", "8", "--steps", "1"])
    assert r.returncode == 2 and "visible" in r.stderr
