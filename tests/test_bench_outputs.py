"""bench.py's --dump-outputs and --full: what a plain run writes and leaves out.
The dump helper and the argument defaults on the CPU; one small plain run of
the benchmark itself on the GPU, its dump against the same compute_rhs called
here on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_defaults_are_a_plain_run(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_whole_vector(tmp_path):
    v = torch.arange(1000, dtype=torch.float64) * 0.5
    bench.dump_outputs(str(tmp_path / "out"), v, 0, 1)
    got = np.load(tmp_path / "out" / "compute_rhs.npy")
    assert got.dtype == np.float64 and np.array_equal(got, v.numpy())
    bench.dump_outputs(str(tmp_path / "out"), v, 1, 2)
    assert np.array_equal(np.load(tmp_path / "out" / "compute_rhs_rank1.npy"), v.numpy())


def test_dump_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8 * 256)
    v = torch.arange(5000, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "a"), v, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), v, 0, 1)
    a, b = np.load(tmp_path / "a" / "compute_rhs.npy"), np.load(tmp_path / "b" / "compute_rhs.npy")
    assert a.shape == (256,) and np.array_equal(a, b)
    # entries of v at sorted indices (v[i] = i), spread over the whole vector
    assert np.all(np.diff(a) >= 0) and np.all(a == np.floor(a)) and a[0] < 500 and a[-1] >= 4500
    # every rank's file together stays within the limit
    bench.dump_outputs(str(tmp_path / "c"), v, 3, 4)
    assert np.load(tmp_path / "c" / "compute_rhs_rank3.npy").shape == (64,)


@pytest.mark.gpu
def test_plain_run_dumps_last_step(tmp_path):
    n, p = 47, 5
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--settle-ms", "0", "--n", str(n), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["settle_steps"] == 0
    assert line["ms_per_step"] > 0 and line["unit"] == "DoF-updates/s" and line["dtype"] == "f64"
    assert line["value"] == pytest.approx(line["config"]["n_dofs_global"] / (line["ms_per_step"] * 1e-3))
    # a plain run leaves every other leg out
    for key in ("rk4_stage_ms", "c3_per_rank_8", "c4_wave", "cpu_baseline"):
        assert line[key] is None
    assert line["roofline"]["traffic"] is None and line["roofline"]["mass_solve"] is None
    assert os.listdir(tmp_path) == ["compute_rhs.npy"]
    got = np.load(tmp_path / "compute_rhs.npy")
    assert got.dtype == np.float64 and got.shape == ((n + 1) ** 3,)

    # the same compute_rhs on the benchmark's inputs (same seeds, same order of draws)
    from gdm_amd import GdmOperator

    op = GdmOperator(3, p, (n, n, n), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), "advection", params=(1.0, 0.15, -0.05))
    gen = torch.Generator(device="cuda").manual_seed(20251010)
    src = torch.rand(op.n_local, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    dst = op.new_vector(local=False)
    bc = torch.rand(op.n_bc_points, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    op.apply(src, dst, bc)
    torch.cuda.synchronize()
    assert np.array_equal(got, dst.cpu().numpy())
