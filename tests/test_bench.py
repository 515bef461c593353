"""bench.py's command line: a plain run prints the headline alone, --full adds the secondary records, --dump-outputs writes what
the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
SECONDARY = ("roofline", "amp_bf16", "fp32_bf16x3", "device_input", "models", "comm", "cpu_baseline")


def _bench(*args, timeout=60):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), cwd=ROOT, capture_output=True, text=True,
                          timeout=timeout)


def test_dump_outputs_writes_float_arrays_with_fixed_samples(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LOGIT_ROWS", 64)
    monkeypatch.setattr(bench, "DUMP_PARAM_ENTRIES", 100)
    torch.manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(30, 5)), torch.nn.Parameter(torch.randn(7)), torch.nn.Parameter(torch.randn(3))]
    for p in params[:2]:
        p.grad = torch.randn_like(p)
    out = {"logits": torch.randn(200, 20).to(torch.bfloat16), "loss": torch.tensor(1.5)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out, params)
    names = {"loss", "logits", "grads", "weights", "grad_norms"}
    assert {f[:-4] for f in os.listdir(tmp_path / "a")} == names
    for n in names:
        a, b = np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))
        assert a.dtype in (np.float32, np.float64), n
        assert np.array_equal(a, b), n      # the same sample in every run
    assert np.load(tmp_path / "a" / "logits.npy").shape == (64, 20)
    assert np.load(tmp_path / "a" / "grads.npy").shape == (100,)
    norms = np.load(tmp_path / "a" / "grad_norms.npy")
    assert norms.dtype == np.float64 and norms.shape == (3,) and norms[2] == 0.0   # a parameter without a gradient: zeros
    assert np.isclose(norms[0], float(params[0].grad.double().norm()))
    flat_w = torch.cat([p.detach().flatten() for p in params]).numpy()
    assert np.isin(np.load(tmp_path / "a" / "weights.npy"), flat_w).all()
    # at the bench's own sizes the files stay far below 64 MB
    assert (bench.DUMP_LOGIT_ROWS * 20 + 2 * bench.DUMP_PARAM_ENTRIES) * 4 < 64 << 20


def test_secondary_record_options_need_full():
    for extra in (["--device-input"], ["--models", "minkunet18"], ["--steps", "0"]):
        r = _bench("--gpus", "1", *extra)
        assert r.returncode == 2, (extra, r.stderr[-500:])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_outputs(tmp_path, hip):
    r = _bench("--gpus", "1", "--steps", "2", "--warmup", "1", "--frames-per-gpu", "2", "--dump-outputs", str(tmp_path),
               timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert all(k in res for k in HEADLINE), res
    assert res["steps"] == 2 and res["warmup"] == 1 and res["dtype"] == "f32" and res["ms_per_step"] > 0
    assert abs(res["value"] - 2 * 1e3 / res["ms_per_step"]) <= 0.01 * res["value"]
    assert not any(k in res for k in SECONDARY), res
    files = sorted(os.listdir(tmp_path))
    assert files == ["grad_norms.npy", "grads.npy", "logits.npy", "loss.npy", "weights.npy"], files
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 64 << 20
    loss = np.load(tmp_path / "loss.npy")
    assert loss.dtype == np.float32 and abs(float(loss[0]) - res["config"]["loss"]) <= 1e-4 * max(1.0, abs(float(loss[0])))
    logits = np.load(tmp_path / "logits.npy")
    assert logits.dtype == np.float32 and logits.shape[1] == 20 and np.isfinite(logits).all()
