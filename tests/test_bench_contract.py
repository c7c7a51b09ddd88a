"""bench.py driver contract: single- and multi-rank (gloo) CPU sanity.

The driver launches `torch.distributed.run --nproc-per-node N bench.py` for
the scaling benchmark; this guards that path (rank env handling, gloo init,
max-over-ranks timing, single rank-0 JSON line) without a GPU.
"""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse_json_line(stdout: str) -> dict:
    lines = [l for l in stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, f"expected exactly one JSON line, got: {stdout!r}"
    return json.loads(lines[0])


def test_bench_single_rank_cpu():
    r = subprocess.run(
        [sys.executable, "bench.py", "--device", "cpu", "--steps", "3",
         "--warmup", "2", "--vus", "4", "--max-turns", "2"],
        cwd=ROOT, capture_output=True, text=True, timeout=300,
    )
    assert r.returncode == 0, r.stderr[-2000:]
    d = _parse_json_line(r.stdout)
    assert d["n_gpus"] == 1 and d["steps"] == 3
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert d["higher_is_better"] is True
    assert d["scaling"] == "weak"
    assert set(d) >= {"metric", "value", "unit", "warmup", "dtype", "data",
                      "config", "vs_baseline"}


def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's outputs as float .npy;
    same arguments -> same inputs -> identical dumps. --full is accepted and
    leaves the result line's contract intact."""
    import numpy as np

    def run(out, *extra):
        r = subprocess.run(
            [sys.executable, "bench.py", "--device", "cpu", "--steps", "3",
             "--warmup", "2", "--vus", "4", "--max-turns", "2",
             "--dump-outputs", str(out), *extra],
            cwd=ROOT, capture_output=True, text=True, timeout=300,
        )
        assert r.returncode == 0, r.stderr[-2000:]
        d = _parse_json_line(r.stdout)
        assert d["steps"] == 3 and d["ms_per_step"] > 0
        return {f: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}

    a = run(tmp_path / "a")
    b = run(tmp_path / "b", "--full")
    assert set(a) == set(b) == {
        "vu_ids.npy", "new_token_ids.npy", "logprobs.npy", "output_token_ids.npy"
    }
    n = a["vu_ids.npy"].shape[0]
    assert n > 0  # the last timed step sampled for at least one request
    for f, x in a.items():
        assert x.dtype in (np.float32, np.float64) and x.shape[0] == n
        np.testing.assert_array_equal(x, b[f])
    assert (a["new_token_ids.npy"] >= 0).all()
    assert np.isfinite(a["logprobs.npy"]).all() and (a["logprobs.npy"] <= 0).all()
    # the step's new token is the last generated token of its request
    gen = a["output_token_ids.npy"]
    last = np.array([row[row >= 0][-1] for row in gen])
    np.testing.assert_array_equal(last, a["new_token_ids.npy"])


def test_bench_two_ranks_gloo():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", str(port), "bench.py", "--gpus", "2",
         "--device", "cpu", "--steps", "3", "--warmup", "2", "--vus", "4",
         "--max-turns", "2"],
        cwd=ROOT, capture_output=True, text=True, timeout=600,
    )
    assert r.returncode == 0, r.stderr[-2000:]
    d = _parse_json_line(r.stdout)
    assert d["n_gpus"] == 2
    # whole-job aggregate: two replicas of fixed per-replica work
    assert d["value"] > 0
