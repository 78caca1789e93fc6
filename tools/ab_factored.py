#!/usr/bin/env python3
"""One H and one A factored once: qpb_solve_factored against qpb_solve_shared,
rounds interleaved as in tools/ab_shared.py (clock and thermal drift hit every
leg alike):
  a   qpb_solve_shared, shared = H | A, on the one copy
  b   qpb_solve_factored on a buffer made outside the timed region
  c   qpb_factor_shared + qpb_solve_factored: what the first solve after a new
      model costs
  python tools/ab_factored.py N M B OUT.json
H0 and A0 are QP 0 of qpb_generate's dense family, f and b every QP's own
(b > 0: x = 0 is feasible for every QP) -- tools/ab_shared.py's inputs.  Per leg:
the median and minimum over all launches, the median of each round and their
spread (max - min).  The bar is against leg a of the same run: b must be faster
than a by more than three times the spread of a's round medians.
Checked at this size: status and active of leg b equal leg a's, the worst
|x_b - x_a| / (1 + max|x_a|) over the batch, and how many QPs differ in iters.
env: ROUNDS (5), REPS (6) -- 30 timed samples per leg; INNER (1): launches per
timed sample, back to back between one pair of events, the time reported per
launch -- a sample of one 0.15 ms launch is mostly the clock's and the
scheduler's noise, a sample of 16 is not"""
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
    sol_a = qpb.solve_shared(H0, f, A0, b, 0)
    F = qpb.factor_shared(H0, A0)
    sol_b = qpb.solve_factored(F, f, b, 0)
    sol_c = qpb.solve_factored(F, f, b, 0)
    s = torch.cuda.current_stream()
    legs = {
        "a": lambda: qpb.solve_shared(H0, f, A0, b, 0, out=sol_a),
        "b": lambda: qpb.solve_factored(F, f, b, 0, out=sol_b),
        "c": lambda: qpb.solve_factored(qpb.factor_shared(H0, A0), f, b, 0, out=sol_c),
    }
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
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
           "factor_doubles": qpb.factor_doubles(n, m), "factor_status": int(F.status.item()),
           "status_counts": torch.bincount(sol_b.status, minlength=5).tolist(), "legs": {}}
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
    # ---- the outputs at this size
    torch.cuda.synchronize()
    rel = (sol_b.x - sol_a.x).abs().amax(1) / (1.0 + sol_a.x.abs().amax(1))
    res["checks"] = {
        "status_equal": bool(torch.equal(sol_a.status, sol_b.status)),
        "active_equal_qps": int((sol_a.active == sol_b.active).all(1).sum()),
        "iters_differ_qps": int((sol_a.iters != sol_b.iters).sum()),
        "x_worst_rel": float(rel.max()),
        "c_bitwise_b": bool(torch.equal(sol_b.x.view(torch.int64), sol_c.x.view(torch.int64))),
    }
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
