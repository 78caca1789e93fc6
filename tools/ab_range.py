#!/usr/bin/env python3
"""Timing of qpb_solve_range against the pair rewrite it replaces, on the same
QPs, rounds interleaved as in tools/ab_eq.py (clock and thermal drift hit every
leg alike):
  range  qpb_solve_range(A, bl, bu)            a two-sided row as one row
  pairs  qpb_solve on [A; -A], [bu; -bl]       each row as two inequalities (2 m rows)
  plain  qpb_solve on (A, bu)                  the upper sides alone: the scale
  python tools/ab_range.py N M B OUT.json
The QPs are qpb_generate's dense family (x = 0 strictly feasible, bu >= 1) with
bl = -(bu of the rows in reverse order): x = 0 stays strictly feasible and the
lower sides have the upper sides' distribution, so both sides end up active
about equally often (the counts are recorded).
Per leg: the median and minimum over all launches, the median of each round
and their spread (max - min), the noise a difference has to clear: a
difference counts when it exceeds three times the spread of the pairs leg.
Iterations per QP and the statuses of every leg are recorded, and x of range
and pairs are compared.
env: ROUNDS (5), REPS (6)"""
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
    H, f, A, bu = qpb.generate(n, B, 1, family="dense", m=m, shift=1.0, box=10.0, device=dev)
    bl = -bu.flip(1).contiguous()
    A2 = torch.cat([A, -A], dim=1).contiguous()
    b2 = torch.cat([bu, -bl], dim=1).contiguous()
    legs = {
        "range": lambda o: qpb.solve_range(H, f, A, bl, bu, out=o),
        "pairs": lambda o: qpb.solve(H, f, A2, b2, out=o),
        "plain": lambda o: qpb.solve(H, f, A, bu, out=o),
    }
    sols = {nm: fn(None) for nm, fn in legs.items()}
    for nm, fn in legs.items():
        for _ in range(3):
            fn(sols[nm])
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    times = {nm: [] for nm in legs}
    rmed = {nm: [] for nm in legs}
    for _ in range(rounds):
        for nm, fn in legs.items():
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                fn(sols[nm])
                e1.record(s)
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            times[nm] += ts
            rmed[nm].append(sorted(ts)[len(ts) // 2])
    res = {"n": n, "m": m, "B": B, "rounds": rounds, "reps": reps, "library": qpb.version()[:8],
           "rows": {"range": m, "pairs": 2 * m, "plain": m}, "legs": {}}
    for nm in legs:
        t = sorted(times[nm])
        st = sols[nm].status
        res["legs"][nm] = {"median_ms": t[len(t) // 2], "min_ms": t[0], "round_medians_ms": rmed[nm],
                           "spread_ms": max(rmed[nm]) - min(rmed[nm]),
                           "status_counts": torch.bincount(st, minlength=5).tolist(),
                           "mean_iters": float(sols[nm].iters.double().mean())}
    rows = torch.arange(m, device=dev)
    bits = lambda words: ((words[:, rows // 32] >> (rows % 32)) & 1).sum().item()  # noqa: E731
    act, low = bits(sols["range"].active), bits(sols["range"].lower)
    res["range_active_rows_per_qp"] = {"upper": (act - low) / B, "lower": low / B}
    xr, xp = sols["range"].x, sols["pairs"].x
    ok = (sols["range"].status == 0) & (sols["pairs"].status == 0)
    rel = (xr - xp).abs().amax(1) / xp.abs().amax(1).clamp(min=1.0)
    res["range_vs_pairs_max_rel_x"] = float(rel[ok].max()) if bool(ok.any()) else None
    res["all_ok"] = bool(ok.all())
    res["range_over_pairs"] = res["legs"]["range"]["median_ms"] / res["legs"]["pairs"]["median_ms"]
    res["range_over_plain"] = res["legs"]["range"]["median_ms"] / res["legs"]["plain"]["median_ms"]
    diff = res["legs"]["pairs"]["median_ms"] - res["legs"]["range"]["median_ms"]
    res["pairs_minus_range_ms"] = diff
    res["difference_counts"] = abs(diff) > 3.0 * res["legs"]["pairs"]["spread_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
