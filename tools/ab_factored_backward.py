#!/usr/bin/env python3
"""The backward on one H and one A factored once: qpb_solve_factored_backward
against qpb_solve_shared_backward, rounds interleaved as in tools/ab_factored.py
(clock and thermal drift hit every leg alike):
  a    qpb_solve_shared_backward, shared = H | A, all four gradients
  b    qpb_solve_factored_backward on a buffer made outside the timed region
  c    qpb_factor_shared_backward + qpb_solve_factored_backward: what the
       backward of a QP layer costs (a new H and A every step)
  a1   leg a with need = (f, b): pass 1 alone, the kernels that differ
  b1   leg b with need = (f, b)
  python tools/ab_factored_backward.py N M B OUT.json
The inputs are tools/ab_shared.py's: H0 and A0 are QP 0 of qpb_generate's dense
family, f and b every QP's own, the solution a forward qpb_solve_shared's, the
cotangent seeded.  Per leg: the median and minimum over all launches, the
median of each round and their spread (max - min).  The bar is against leg a
of the same run: b must be faster than a by more than three times the spread
of a's round medians (and b1 against a1 likewise).
Checked at this size: every output of leg b, c and b1 equals leg a's bit for bit.
env: ROUNDS (5), REPS (6) -- 30 timed samples per leg; INNER (1): launches per
timed sample, back to back between one pair of events, the time reported per
launch"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "embedded-qp-solver_amd"))
import torch  # noqa: E402

import qpb  # noqa: E402


def main(n, m, B, out_path):
    dev = torch.device("cuda", 0)
    rounds, reps = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("REPS", 6))
    inner = int(os.environ.get("INNER", 1))
    H, f, A, b = qpb.generate(n, B, 1, family="dense", m=m, shift=1.0, box=10.0, device=dev)
    H0, A0 = H[0].clone(), A[0].clone()
    del H, A
    sol = qpb.solve_shared(H0, f, A0, b, 0)
    gx = torch.randn(B, n, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    F = qpb.factor_shared_backward(H0, A0)
    fb = ("f", "b")
    legs = {
        "a": lambda: qpb.solve_shared_backward(H0, A0, sol, gx),
        "b": lambda: qpb.solve_factored_backward(F, sol, gx),
        "c": lambda: qpb.solve_factored_backward(qpb.factor_shared_backward(H0, A0), sol, gx),
        "a1": lambda: qpb.solve_shared_backward(H0, A0, sol, gx, need=fb),
        "b1": lambda: qpb.solve_factored_backward(F, sol, gx, need=fb),
    }
    s = torch.cuda.current_stream()
    outs = {}
    for nm, fn in legs.items():
        for _ in range(3):
            outs[nm] = fn()
    torch.cuda.synchronize()
    same = lambda p, q: all((u is None and v is None) or torch.equal(u.view(torch.int64), v.view(torch.int64))  # noqa: E731
                            for u, v in zip(p, q))
    checks = {"b_bitwise_a": bool(same(outs["b"], outs["a"])), "c_bitwise_a": bool(same(outs["c"], outs["a"])),
              "b1_bitwise_a1": bool(same(outs["b1"], outs["a1"])),
              "a1_bitwise_a": bool(same(outs["a1"][1::2], outs["a"][1::2])),
              "finite": bool(all(torch.isfinite(t).all() for t in outs["b"]))}
    del outs
    times = {nm: [] for nm in legs}
    rmed = {nm: [] for nm in legs}
    for _ in range(rounds):
        for nm, fn in legs.items():
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for _ in range(inner):
                    fn()
                e1.record(s)
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) / inner)
            times[nm] += ts
            rmed[nm].append(sorted(ts)[len(ts) // 2])
    res = {"n": n, "m": m, "B": B, "rounds": rounds, "reps": reps, "inner": inner, "library": qpb.version()[:8],
           "factor_backward_doubles": qpb.factor_backward_doubles(n, m), "factor_status": int(F.status.item()),
           "status_counts": torch.bincount(sol.status, minlength=5).tolist(), "legs": {}}
    for nm in legs:
        t = sorted(times[nm])
        res["legs"][nm] = {"median_ms": t[len(t) // 2], "min_ms": t[0], "round_medians_ms": rmed[nm],
                           "spread_ms": max(rmed[nm]) - min(rmed[nm])}
    L = res["legs"]
    res["a_minus_b_ms"] = L["a"]["median_ms"] - L["b"]["median_ms"]
    res["b_over_a"] = L["b"]["median_ms"] / L["a"]["median_ms"]
    res["factor_once_ms_c_minus_b"] = L["c"]["median_ms"] - L["b"]["median_ms"]
    res["bar_ms_3_spreads_of_a"] = 3 * L["a"]["spread_ms"]
    res["clears_bar"] = bool(res["a_minus_b_ms"] > res["bar_ms_3_spreads_of_a"])
    res["pass1_a1_minus_b1_ms"] = L["a1"]["median_ms"] - L["b1"]["median_ms"]
    res["pass1_b1_over_a1"] = L["b1"]["median_ms"] / L["a1"]["median_ms"]
    res["pass1_bar_ms_3_spreads_of_a1"] = 3 * L["a1"]["spread_ms"]
    res["pass1_clears_bar"] = bool(res["pass1_a1_minus_b1_ms"] > res["pass1_bar_ms_3_spreads_of_a1"])
    res["checks"] = checks
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
