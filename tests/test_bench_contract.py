"""bench.py driver-contract test: runs the real script (CPU, tiny) and
validates the JSON line fields the driver parses."""
import json
import os
import subprocess
import sys

import pytest

# The multi-rank tests below are gloo-on-CPU runs (several ranks cannot share
# one GPU under RCCL) and the exact dump comparison needs the bit-reproducible
# CPU path (no atomics): their child processes see no GPU even where one exists.
CPU_ENV = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")


def test_bench_json_contract():
    out = subprocess.run(
        [sys.executable, "bench.py", "--steps", "2", "--warmup", "1",
         "--batch", "32", "--vocab", "1000", "--n-cat", "4"],
        capture_output=True, text=True, timeout=600, env=CPU_ENV)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.strip().splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
              "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config"):
        assert k in d, f"missing field {k}"
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True
    assert d["scaling"] == "weak"
    assert d["data"] == "synthetic"
    assert d["value"] > 0
    assert "global_batch" in d["config"] and "parallelism" in d["config"]


DUMP_FILES = ["dense_index.npy", "dense_params.npy", "emb0_adagrad.npy",
              "emb0_rows.npy", "emb0_weights.npy", "logits.npy", "loss.npy"]


def _dump_run(out_dir, batch, steps, env=None):
    """bench.py at a tiny size with --dump-outputs -> (result line, arrays);
    checks the files' names, dtypes and shapes."""
    import numpy as np
    out = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--vocab", "1000",
         "--n-cat", "4", "--warmup", "1", "--steps", str(steps),
         "--batch", str(batch), "--dump-outputs", str(out_dir)],
        capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == "samples_per_sec_wide_deep" and d["ms_per_step"] > 0
    assert d["steps"] == steps
    a = {p.name: np.load(p) for p in sorted(out_dir.glob("*.npy"))}
    assert sorted(a) == DUMP_FILES
    for name, v in a.items():
        assert v.dtype in (np.float32, np.float64), (name, v.dtype)
        assert np.isfinite(v).all(), name
    rows = min(batch, 256) * 4      # sampled batch rows x features
    assert a["loss.npy"].shape == (1,) and a["loss.npy"].dtype == np.float32
    assert a["logits.npy"].shape == (batch,)
    assert a["dense_index.npy"].shape == a["dense_params.npy"].shape == (65536,)
    assert a["emb0_rows.npy"].shape == (rows,)
    assert a["emb0_weights.npy"].shape == (rows, 64 + 1)
    assert a["emb0_adagrad.npy"].shape == (rows,)
    assert sum(v.nbytes for v in a.values()) <= 64 * 2**20
    # sigmoid cross-entropy of a barely trained model sits near ln 2
    assert 0.0 < float(a["loss.npy"][0]) < 5.0
    # every dumped row was looked up by the last batch, so rowwise adagrad
    # has accumulated a positive squared gradient in each of them
    assert (a["emb0_adagrad.npy"] > 0).all()
    return d, a


def test_bench_dump_outputs_cpu(tmp_path):
    """--dump-outputs writes the last timed step's results as float .npy
    files, identically for two runs with the same arguments (seeded inputs,
    deterministic CPU path)."""
    import numpy as np
    da, a = _dump_run(tmp_path / "a", 32, 2, CPU_ENV)
    db, b = _dump_run(tmp_path / "b", 32, 2, CPU_ENV)
    dc, c = _dump_run(tmp_path / "c", 32, 3, CPU_ENV)
    assert da["dtype"] == "fp32"
    for name in DUMP_FILES:
        assert np.array_equal(a[name], b[name]), name
    # --steps really sets the number of timed steps: the third step sees
    # another batch and moved-on parameters
    assert np.array_equal(a["dense_index.npy"], c["dense_index.npy"])
    for name in ("loss.npy", "logits.npy", "dense_params.npy"):
        assert not np.array_equal(a[name], c[name]), name


def test_bench_full_flag():
    """--full is accepted and keeps the result line's contract."""
    out = subprocess.run(
        [sys.executable, "bench.py", "--steps", "2", "--warmup", "1",
         "--batch", "32", "--vocab", "1000", "--n-cat", "4", "--full"],
        capture_output=True, text=True, timeout=600, env=CPU_ENV)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == "samples_per_sec_wide_deep" and d["unit"] == "samples/s"
    assert d["steps"] == 2 and d["ms_per_step"] > 0


@pytest.mark.gpu
def test_bench_dump_outputs_gpu(tmp_path):
    """GPU (bf16, hipGraph) path of --dump-outputs at a tiny size: the
    graph's static loss/logits buffers after the last replay and the bf16
    unified arena (in-row accumulator bits decoded), written by two runs.

    Run-to-run bound on the loss: it is an f32 mean over logits that the
    kernels round to bf16, and two runs differ only in the order of atomic
    accumulation, so one bf16 rounding step (2^-8 = 3.9e-3 relative) bounds
    the difference.  Measured on an MI355X: six runs spread over 4.8e-4
    relative (0.99364 .. 0.99411), single logits differ by up to 0.031.
    The other arrays are checked for form only: their element-wise spread
    is not bounded by rounding (bench.py dump_outputs docstring)."""
    import numpy as np
    da, a = _dump_run(tmp_path / "a", 512, 3)
    db, b = _dump_run(tmp_path / "b", 512, 3)
    assert da["dtype"] == "bf16" and da["config"]["hipgraphs"] is True
    for name in ("dense_index.npy", "emb0_rows.npy"):
        assert np.array_equal(a[name], b[name]), name
    la, lb = float(a["loss.npy"][0]), float(b["loss.npy"][0])
    print("loss", la, lb, "max logit diff",
          float(np.abs(a["logits.npy"] - b["logits.npy"]).max()))
    assert abs(la - lb) <= 2.0 ** -8 * abs(la), (la, lb)


def test_bench_torchrun_2rank_contract():
    """The driver's multi-GPU launch path: torchrun world=2 (gloo on CPU),
    EP embeddings, JSON from rank 0 only."""
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29651", "bench.py", "--steps", "2", "--warmup", "1",
         "--batch", "32", "--vocab", "1000", "--n-cat", "4"],
        capture_output=True, text=True, timeout=900, env=CPU_ENV)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, f"expected exactly one JSON line, got {len(lines)}"
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2
    assert d["config"]["global_batch"] == 64
    assert "ep2" in d["config"]["parallelism"]


def test_bench_torchrun_2rank_dp_mode():
    """--emb-mode dp at world=2: replicated arenas + sparse allgather
    aggregation through the real bench script."""
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29653", "bench.py", "--steps", "2", "--warmup", "1",
         "--batch", "32", "--vocab", "1000", "--n-cat", "4",
         "--emb-mode", "dp"],
        capture_output=True, text=True, timeout=900, env=CPU_ENV)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["config"]["parallelism"] == "dp2"
    assert d["value"] > 0


def test_bench_torchrun_4rank_table_ep():
    """world=4 (gloo CPU): the table-EP feature assignment puts 1 feature on
    each of 4 ranks for n-cat=4 — a different split shape than the 2-rank
    tests; exactly what the driver's SCALE run exercises at N=4."""
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
         "--master-port", "29655", "bench.py", "--steps", "2", "--warmup", "1",
         "--batch", "16", "--vocab", "500", "--n-cat", "6"],
        capture_output=True, text=True, timeout=900, env=CPU_ENV)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 4
    assert "ep4" in d["config"]["parallelism"]


def test_bench_torchrun_8rank_table_ep():
    """world=8 (gloo CPU): the driver's SCALE shape at N=8.  With n-cat=26
    (the headline feature count) the greedy assignment puts 3-4 tables on
    each rank; checks the full 8-way static all-to-all path end to end."""
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
         "--master-port", "29657", "bench.py", "--steps", "2", "--warmup", "1",
         "--batch", "16", "--vocab", "200", "--n-cat", "26"],
        capture_output=True, text=True, timeout=900, env=CPU_ENV)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8
    assert d["config"]["global_batch"] == 128
    assert "ep8" in d["config"]["parallelism"]


def test_bench_torchrun_2rank_ep_row():
    """--emb-mode ep_row at world=2: row%world-sharded arenas through the
    real bench script (the beyond-HBM single-table layout)."""
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29659", "bench.py", "--steps", "2", "--warmup", "1",
         "--batch", "32", "--vocab", "1000", "--n-cat", "4",
         "--emb-mode", "ep_row"],
        capture_output=True, text=True, timeout=900, env=CPU_ENV)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2
