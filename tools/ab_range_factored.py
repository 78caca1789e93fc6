#!/usr/bin/env python3
"""Two-sided rows on a factor buffer: qpb_solve_range_factored against
qpb_solve_range with one shared H and A, rounds interleaved as in
tools/ab_factored.py (clock and thermal drift hit every leg alike):
  a   qpb_solve_range, shared = H | A, on the one copy
  b   qpb_solve_range_factored on a buffer made outside the timed region
  c   qpb_factor_shared + qpb_solve_range_factored: what the first solve after a
      new model costs
  d   qpb_solve_factored on (A, bu) alone, the upper sides: the scale
  python tools/ab_range_factored.py N M B OUT.json
H0 and A0 are QP 0 of qpb_generate's dense family, f and bu every QP's own
(bu > 0: x = 0 is feasible for every QP) -- tools/ab_factored.py's inputs -- and
bl = -(bu of the rows in reverse order) as in tools/ab_range.py: x = 0 stays
strictly feasible and the lower sides have the upper sides' distribution.  Per
leg: the median and minimum over all launches, the median of each round and
their spread (max - min).  The bar is against leg a of the same run: b must be
faster than a by more than three times the spread of a's round medians.
Checked at this size: status, active and lower of leg b against leg a's, the
worst |x_b - x_a| / (1 + max|x_a|) over the batch, how many QPs differ in iters,
and the active rows per QP on each side.
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
    H, f, A, bu = qpb.generate(n, B, 1, family="dense", m=m, shift=1.0, box=10.0, device=dev)
    H0, A0 = H[0].clone(), A[0].clone()
    del H, A
    bl = -bu.flip(1).contiguous()
    sol_a = qpb.solve_range(H0, f, A0, bl, bu, 0)
    F = qpb.factor_shared(H0, A0)
    sol_b = qpb.solve_range_factored(F, f, bl, bu, 0)
    sol_c = qpb.solve_range_factored(F, f, bl, bu, 0)
    sol_d = qpb.solve_factored(F, f, bu, 0)
    s = torch.cuda.current_stream()
    legs = {
        "a": lambda: qpb.solve_range(H0, f, A0, bl, bu, 0, out=sol_a),
        "b": lambda: qpb.solve_range_factored(F, f, bl, bu, 0, out=sol_b),
        "c": lambda: qpb.solve_range_factored(qpb.factor_shared(H0, A0), f, bl, bu, 0, out=sol_c),
        "d": lambda: qpb.solve_factored(F, f, bu, 0, out=sol_d),
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
    res["b_over_d"] = L["b"]["median_ms"] / L["d"]["median_ms"]
    res["factor_once_ms_c_minus_b"] = L["c"]["median_ms"] - L["b"]["median_ms"]
    res["bar_ms_3_spreads_of_a"] = 3 * L["a"]["spread_ms"]
    res["clears_bar"] = bool(res["a_minus_b_ms"] > res["bar_ms_3_spreads_of_a"])
    # ---- the outputs at this size
    torch.cuda.synchronize()
    rel = (sol_b.x - sol_a.x).abs().amax(1) / (1.0 + sol_a.x.abs().amax(1))
    rows = torch.arange(m, device=dev)
    bits = lambda words: ((words[:, rows // 32] >> (rows % 32)) & 1).sum().item()  # noqa: E731
    act, low = bits(sol_b.active), bits(sol_b.lower)
    res["checks"] = {
        "status_equal": bool(torch.equal(sol_a.status, sol_b.status)),
        "active_equal_qps": int((sol_a.active == sol_b.active).all(1).sum()),
        "lower_equal_qps": int((sol_a.lower == sol_b.lower).all(1).sum()),
        "iters_differ_qps": int((sol_a.iters != sol_b.iters).sum()),
        "mean_iters": {"a": float(sol_a.iters.double().mean()), "b": float(sol_b.iters.double().mean()),
                       "d": float(sol_d.iters.double().mean())},
        "x_worst_rel": float(rel.max()),
        "c_bitwise_b": bool(torch.equal(sol_b.x.view(torch.int64), sol_c.x.view(torch.int64))),
        "active_rows_per_qp": {"upper": (act - low) / B, "lower": low / B},
    }
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
