"""bench.py as every later change runs it: a plain `--gpus 1 --steps K
--warmup W` run times K steps and leaves the other legs to `--full`, and
`--dump-outputs DIR` writes the last timed step's outputs (a seeded sample of
the QPs) so that two builds can be compared output for output."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FULL_ONLY = ("cpu_baseline", "like_for_like", "box_fast_path", "dense_family", "pipelined", "sustained")


def test_plain_run_dumps_what_the_solver_returns(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    total, seed = 100000, 7  # more QPs than one dump holds at n = 16: the sampled path
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--global-batch", str(total), "--seed", str(seed), "--dump-outputs", str(tmp_path / "dump")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0.0
    assert line["value"] == pytest.approx(total / (line["ms_per_step"] * 1e-3))
    assert line["unit"] == "QPs/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["solver_stats"]["ok_frac"] == 1.0
    assert all(line[k] is None for k in FULL_ONLY)

    idx = bench.dump_sample(total, seed, 16, 32)
    assert 0 < len(idx) < total
    got = {k: np.load(tmp_path / "dump" / f"{k}.npy") for k in ("qp_index", "x", "lam", "active", "status", "iters")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert np.array_equal(got["qp_index"], idx.astype(np.float64))
    # the same QPs (qpb_generate is keyed by seed and QP index) through the same call
    H, f, A, b = qpb.generate(16, total, seed, family="box", shift=1.0, box=10.0)
    sol = qpb.solve(H, f, A, b)
    torch.cuda.synchronize()
    assert np.array_equal(got["x"], sol.x.cpu().numpy()[idx])
    assert np.array_equal(got["lam"], sol.lam.cpu().numpy()[idx])
    assert np.array_equal(got["active"], sol.active.cpu().numpy()[idx].view(np.uint32).astype(np.float64))
    assert np.array_equal(got["status"], sol.status.cpu().numpy()[idx].astype(np.float64))
    assert np.array_equal(got["iters"], sol.iters.cpu().numpy()[idx].astype(np.float64))
