"""The N>1 path on CPU: two ranks over gloo (torch.distributed.run, 127.0.0.1).

1. bench.py --sharded --backend emu: the real bench driver -- every rank generating and aligning the chunk of the config-4
   table it owns (emulated kernels in place of the GPU), rank 0 gathering records and CIGARs with dist.gather of uint8 tensors
   inside the timed loop -- must print one JSON line whose job total scales with the number of ranks.
2. a bespoke worker that compares the gathered records with the unsharded run, job for job.
3. bench.py's plain line and --dump-outputs (emulated, and once on the GPU against the reference's digest).
No data-path collective exists in the product (jobs are independent)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torchrun(args, port):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port)] + args
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)


def test_two_rank_gloo_bench_sharded(emu, hip_lib):
    p = _torchrun([os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--sharded", "--backend", "emu"], 29519)
    assert p.returncode == 0, p.stderr[-3000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1, p.stdout[-2000:]
    rec = json.loads(line[0])
    assert rec["mode"] == "sharded" and rec["n_gpus"] == 2 and rec["scaling"] == "weak" and rec["value"] > 0
    assert rec["config"]["jobs_total"] == 2 * 48 and rec["config"]["jobs_per_gpu"] == 48 and rec["sum_score1"] > 0      # 48 jobs per rank (emu rehearsal)
    assert "f16" in rec["dtype"]


def test_two_rank_gloo_shard_and_gather(emu, tmp_path):
    out = tmp_path / "result.txt"
    p = _torchrun([os.path.join(ROOT, "tests", "dist_worker.py"), str(out)], 29517)
    assert p.returncode == 0, p.stderr[-2000:]
    assert out.read_text().startswith("OK 14")


def test_single_process_bench_drives_every_gpu_from_its_own_host_thread(emu, hip_lib):
    """plain `python bench.py --gpus N` (no torchrun): one host thread per GPU issues that GPU's steps; rehearsed on the emulator.  The
    line names the threads and the measured enqueue cost per GPU, and shard 0's results are those of the one-GPU run."""
    def run(n):
        env = dict(os.environ, PYTHONPATH=ROOT)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--backend", "emu", "--steps", "2", "--warmup", "1",
                            "--reads-per-gpu", "48", "--no-cpu-baseline", "--no-subconfigs", "--streams", "2", "--full"], env=env, capture_output=True, text=True,
                           timeout=900)
        assert p.returncode == 0, p.stderr[-3000:]
        line = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(line) == 1, p.stdout[-2000:]
        return json.loads(line[0])
    one, three = run(1), run(3)
    assert three["n_gpus"] == 3 and three["host_threads"] == 3 and len(three["host_enqueue_ms_per_step"]) == 3
    assert one["host_threads"] == 1 and three["sum_score1"] == one["sum_score1"] > 0


def test_plain_bench_line_and_dumped_outputs(emu, hip_lib, tmp_path):
    """a plain run (no --full) prints the headline line and nothing measured beside it; --dump-outputs writes the last step's records and
    CIGARs as float .npy files, the same from run to run, and they are what the --full run checks (its sum_score1)"""
    def run(out, *extra):
        env = dict(os.environ, PYTHONPATH=ROOT)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--backend", "emu", "--steps", "3", "--warmup", "1",
                            "--reads-per-gpu", "48", "--streams", "2", "--dump-outputs", str(out)] + list(extra),
                           env=env, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-3000:]
        line = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(line) == 1, p.stdout[-2000:]
        return json.loads(line[0])
    a, b = run(tmp_path / "a"), run(tmp_path / "b")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in a, k
    assert a["steps"] == 3 and a["warmup"] == 1 and a["value"] > 0 and a["ms_per_step"] > 0 and a["higher_is_better"] is True
    for k in ("configs", "roofline", "kernel_ms_per_step", "digest", "sum_score1", "cpu_baseline", "small_call", "sustained", "many_loci"):
        assert k not in a, k
    assert a["outputs"]["jobs"] == a["outputs"]["jobs_written"] == 48 and not a["outputs"]["sampled"]
    names = sorted(f for f in os.listdir(tmp_path / "a"))
    assert names == sorted(a["outputs"]["files"]) and "cigar_ops.npy" in names and "score1.npy" in names
    import numpy as np
    for f in names:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), f
    assert len(np.load(tmp_path / "a" / "score1.npy")) == 48
    assert len(np.load(tmp_path / "a" / "cigar_ops.npy")) == int(np.load(tmp_path / "a" / "cigar_len.npy").sum()) > 0
    full = run(tmp_path / "c", "--full", "--no-cpu-baseline")
    assert full["sum_score1"] == int(np.load(tmp_path / "a" / "score1.npy").sum()) > 0


def test_dump_outputs_writes_cigars_in_job_order_and_samples_past_its_budget(tmp_path, monkeypatch):
    """bench.dump_outputs: every job's CIGAR ops in job order whatever the pool layout; past the budget a fixed seeded sample of the jobs,
    the same from call to call, each sampled job with its own fields and ops"""
    import numpy as np
    import bench
    from indelpost_amd._lib import RESULT_DTYPE
    from indelpost_amd.batch import BatchResult
    rng = np.random.default_rng(3)
    n = 5000
    rec = np.zeros(n, RESULT_DTYPE)
    rec["score1"] = rng.integers(0, 450, n)
    rec["ref_end1"] = rng.integers(0, 300, n)
    rec["cigar_len"] = rng.integers(0, 7, n)
    ops = [(rng.integers(1, 150, int(c)) << 4) | rng.integers(0, 3, int(c)) for c in rec["cigar_len"]]
    pool, at = [], 0
    for i in range(n - 1, -1, -1):                     # the pool holds the last job's ops first
        rec["cigar_off"][i] = at
        pool.extend(ops[i].tolist())
        at += len(ops[i])
    res = BatchResult(rec, np.array(pool, np.uint32))
    info = bench.dump_outputs(str(tmp_path / "all"), [res])
    assert not info["sampled"] and info["jobs_written"] == n and "job_index.npy" not in info["files"]
    got = np.load(tmp_path / "all" / "cigar_ops.npy")
    assert got.dtype == np.float32 and np.array_equal(got, np.concatenate(ops).astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "all" / "score1.npy"), rec["score1"].astype(np.float32))

    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 40000)
    one = bench.dump_outputs(str(tmp_path / "s1"), [res])
    two = bench.dump_outputs(str(tmp_path / "s2"), [res])
    assert one["sampled"] and one == two and 0 < one["jobs_written"] < n and one["bytes"] <= 40000
    idx = np.load(tmp_path / "s1" / "job_index.npy").astype(np.int64)
    assert np.array_equal(idx, np.load(tmp_path / "s2" / "job_index.npy")) and (np.diff(idx) > 0).all()
    assert np.array_equal(np.load(tmp_path / "s1" / "ref_end1.npy"), rec["ref_end1"][idx].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "s1" / "cigar_ops.npy"), np.concatenate([ops[i] for i in idx]).astype(np.float32))


@pytest.mark.gpu
def test_dumped_outputs_of_the_headline_equal_the_reference(hip_lib, tmp_path):
    """a plain `bench.py --gpus 1 --dump-outputs DIR` on the GPU: the dumped records and CIGARs of the headline workload, put back into
    a BatchResult, have the digest of the reference's own results on that table (tests/golden/bench_digests.json)"""
    import numpy as np
    from indelpost_amd._lib import RESULT_DTYPE
    from indelpost_amd.batch import BatchResult
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out)],
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 2 and line["outputs"]["jobs"] == 1000000 and not line["outputs"]["sampled"]
    rec = np.zeros(1000000, RESULT_DTYPE)
    for f in ("score1", "score2", "ref_begin1", "ref_end1", "read_begin1", "read_end1", "ref_end2", "flag", "cigar_len"):
        a = np.load(out / (f + ".npy"))
        assert a.dtype in (np.float32, np.float64)
        rec[f] = a
    cl = rec["cigar_len"].astype(np.int64)
    rec["cigar_off"] = np.cumsum(cl) - cl
    ops = np.load(out / "cigar_ops.npy").astype(np.uint32)
    assert len(ops) == int(cl.sum())
    with open(os.path.join(ROOT, "tests", "golden", "bench_digests.json")) as f:
        gold = json.load(f)["workloads"]["2b"]
    assert gold["n_jobs"] == 1000000 and BatchResult(rec, ops).digest() == gold["digest"]
