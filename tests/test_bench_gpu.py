"""The driver-facing bench paths on a GPU: the plain run and its --dump-outputs; the N > 1 launch (one rank per GPU under
torch.distributed.run) with --full and the compact line.
An 8-GPU node is not available to the GPU suite, so two ranks share device 0 and talk over gloo (WFA_BENCH_BACKEND / WFA_BENCH_SHARE_DEVICE,
development aids of bench.py): every line of the N > 1 path runs except RCCL itself."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _strict(line):
    def bad(x):
        raise ValueError(x)
    return json.loads(line, parse_constant=bad)


@pytest.mark.gpu
def test_bench_two_ranks_share_one_device(gpu):
    env = dict(os.environ, WFA_BENCH_BACKEND="gloo", WFA_BENCH_SHARE_DEVICE="1", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(29700 + os.getpid() % 200), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--pairs", "200000", "--c3-pairs", "1000", "--full"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    line = p.stdout.strip().splitlines()[-1]
    assert len(line) < 8000
    r = _strict(line)
    assert r["n_gpus"] == 2 and r["steps"] == 3 and r["warmup"] == 1 and r["scaling"] == "weak" and r["errors"] == []
    assert r["value"] > 0 and r["ms_per_step"] > 0
    # both halves of the metric: 150 bp (value) and 10 kb (the C3 leg every rank runs), summed over the ranks
    assert r["config"]["c3_alignments_per_s"] > 0 and r["config"]["c3_invalid_transcripts"] == 0
    assert "roofline" in r and r["roofline"]["bound"] == "hbm"


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_steps_results(gpu, tmp_path):
    """A plain run (no --full) times exactly --steps steps and carries nothing of --full; --dump-outputs writes the last step's
    per-pair score and status in float64, the oracle's on the same seeded pairs."""
    from oracle import loader
    from pywfa_amd import datagen
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--pairs", "100000",
           "--dump-outputs", str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    r = _strict(p.stdout.strip().splitlines()[-1])
    assert r["n_gpus"] == 1 and r["steps"] == 4 and r["warmup"] == 1 and r["errors"] == []
    assert r["metric"] == "pairwise alignments/sec" and r["unit"] == "alignments/s" and r["higher_is_better"] is True
    assert r["ms_per_step"] > 0 and r["value"] == pytest.approx(100000 / (r["ms_per_step"] * 1e-3), rel=1e-4)
    assert "cpu_baseline" not in r and "end_to_end" not in r and "offsets_per_s" not in r and r["detail"] is None
    assert r["roofline"]["bound"] == "hbm" and r["roofline"]["kernel_ms"] > 0
    score, status = np.load(out / "score.npy"), np.load(out / "status.npy")
    assert score.dtype == np.float64 and status.dtype == np.float64 and len(score) == len(status) == 100000
    batch = datagen.subset(datagen.generate(100000, 150, 0.02, datagen.SEEDS["C2"]), np.arange(2000))
    o = loader.run(loader.oracle(), loader.make_config(span="end-to-end", scope="score"), batch, want_cigar=False)
    assert np.array_equal(score[:2000], o["score"]) and np.array_equal(status[:2000], o["status"])
