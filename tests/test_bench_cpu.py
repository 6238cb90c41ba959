"""CPU: bench.py's options and its output dump (the timed run itself needs a HIP device: tests/test_gpu_bench_contract.py)."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_lists_full_and_dump_outputs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300,
                         cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "--full" in out.stdout and "--dump-outputs" in out.stdout


def test_dump_outputs_writes_losses_and_every_parameter_as_float32(tmp_path):
    spec = importlib.util.spec_from_file_location("_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    net = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.Linear(3, 1))
    losses = torch.tensor([0.5, 0.25], dtype=torch.float32)
    bench.dump_outputs(str(tmp_path / "out"), losses, net)
    files = {p.name: np.load(p) for p in (tmp_path / "out").glob("*.npy")}
    assert set(files) == {"losses.npy", "param.0.weight.npy", "param.0.bias.npy", "param.1.weight.npy", "param.1.bias.npy"}
    assert all(a.dtype == np.float32 for a in files.values())
    assert np.array_equal(files["losses.npy"], losses.numpy())
    assert np.array_equal(files["param.0.weight.npy"], net[0].weight.detach().numpy())
