"""The bench line's contract, checked on CPU against the newest committed line (profiles/r*_bench.json, written by
`python bench.py --full` on an MI355X box) and against bench.py's own argument handling: the keys the driver reads, the
tier's `roofline` / `cpu_baseline` objects, internal consistency of the numbers (value = steps * batch / time, frac =
achieved / peak), and that nothing in bench.py reads the reference's tree or imports the oracle outside the
cpu_baseline leg.
--dump-outputs: the writer on CPU tensors here; a plain run on the GPU (lean line, outputs written, the same outputs
from a second run with the same arguments)."""
import glob
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _newest_line():
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_bench.json")))
    assert files, "no committed bench line under profiles/"
    return files[-1], json.loads(open(files[-1]).read().strip().splitlines()[-1])


def test_committed_bench_line_has_the_contract_keys():
    f, d = _newest_line()
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, (f, k)
    assert d["unit"] == "samples/s" and d["higher_is_better"] is True and d["scaling"] == "weak" and d["data"] == "synthetic"
    assert d["dtype"] == "f32" and d["vs_baseline"] is None and d["n_gpus"] == 1
    assert "workload" in d["config"] and "model" not in d["config"]
    B = d["config"]["global_batch"]
    assert abs(d["value"] - B / (d["ms_per_step"] * 1e-3)) <= 2e-3 * d["value"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) <= 2e-3
    assert 0 < r["step_frac"] < 1
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0


def test_bench_source_keeps_the_oracle_in_the_baseline_leg_and_off_the_reference():
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "/root/reference" not in src
    # every import of the oracle sits inside the cpu_baseline helpers
    for m in re.finditer(r"^(\s*)(from oracle|import oracle)", src, re.M):
        head = src[:m.start()]
        fn = re.findall(r"^def (\w+)\(", head, re.M)[-1]
        assert fn in ("_oracle_step_fn", "cpu_baseline"), fn
    pkg = os.path.join(ROOT, "multimodal_vae_comparison_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                s = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import) oracle", s, re.M), os.path.join(dirpath, f)
                assert "/root/reference" not in s, os.path.join(dirpath, f)


def test_plain_run_and_full_are_separate_options(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 3 and a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_writes_float_arrays_and_samples_large_ones(tmp_path):
    import bench
    big = torch.arange(bench.DUMP_MAX_ELEMS + 1000, dtype=torch.float32).reshape(-1, 8)
    arrays = {"loss": torch.tensor(3.5, dtype=torch.float64), "kld": torch.zeros((), dtype=torch.int64),
              "rec": torch.randn(5, 4).half(), "parameters": big}
    bench.dump_outputs(arrays, str(tmp_path / "a"))
    bench.dump_outputs(arrays, str(tmp_path / "b"))
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(got) == set(arrays)
    assert got["loss"].dtype == np.float64 and got["loss"] == 3.5
    assert got["kld"].dtype == np.float64 and got["rec"].dtype == np.float32 and got["rec"].shape == (5, 4)
    p = got["parameters"]
    assert p.dtype == np.float32 and p.shape == (bench.DUMP_MAX_ELEMS,)
    assert np.all(np.diff(p) > 0) and p[-1] < big.numel()          # sorted distinct elements of the original
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_BUDGET_BYTES
    for name in arrays:                                              # the same sample every time
        assert np.array_equal(got[name], np.load(tmp_path / "b" / (name + ".npy"))), name


@pytest.mark.gpu
def test_plain_bench_run_is_lean_and_dumps_reproducible_outputs(hip_lib, tmp_path):
    """a plain run prints the headline without the --full figures, and two runs with the same arguments write the
    same outputs of the last timed step"""
    lines = []
    for d in ("a", "b"):
        cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2", "--dump-outputs",
               str(tmp_path / d)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, f"--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-3000:]}"
        out = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
        assert len(out) == 1, r.stdout[-2000:]
        lines.append(json.loads(out[0]))
    res = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in res, k
    for k in ("roofline", "cpu_baseline", "spread", "extras", "first_window_ms_per_step"):
        assert k not in res, k
    assert res["steps"] == 5 and res["unit"] == "samples/s" and res["dtype"] == "f32"
    assert abs(res["value"] - res["config"]["global_batch"] / (res["ms_per_step"] * 1e-3)) <= 2e-3 * res["value"]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"loss.npy", "kld.npy", "parameters.npy", "gradients.npy"} <= set(names)
    total = 0
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        total += a.nbytes
        assert a.dtype in (np.float32, np.float64) and a.shape == b.shape and np.isfinite(a).all(), f
        assert np.allclose(a, b, rtol=1e-5, atol=1e-6 * max(1.0, float(np.abs(b).max()))), f
    assert total <= 64 << 20
    assert float(np.load(tmp_path / "a" / "loss.npy")) == pytest.approx(res["final_loss"], abs=1e-3)
