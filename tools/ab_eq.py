#!/usr/bin/env python3
"""Timing of qpb_solve_eq against the two ways of doing without it, on the same
QPs, rounds interleaved as in tools/ab.py (clock and thermal drift hit every
leg alike):
  eq     qpb_solve_eq(meq)                      the equalities as rows 0 .. meq-1
  pairs  qpb_solve on [A; -A[:meq]], [b; -b[:meq]]   each equality as two inequalities (m + meq rows)
  plain  qpb_solve on the generator's QPs       the same shape without equalities: the scale
  python tools/ab_eq.py N M MEQ B OUT.json
The QPs are qpb_generate's dense family (x = 0 strictly feasible, b >= 1) with
b[:meq] = A[:meq] xc, xc ~ U(-0.1, 0.1)^n: xc satisfies the equalities and
keeps a slack of at least 0.6 on every inequality.
Per leg: the median and minimum over all launches, the median of each round
and their spread (max - min), the noise a difference has to clear.  The
outputs of eq and pairs are compared too (statuses, x).
env: ROUNDS (5), REPS (6)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "embedded-qp-solver_amd"))
import torch  # noqa: E402

import qpb  # noqa: E402


def main(n, m, meq, B, out_path):
    dev = torch.device("cuda", 0)
    rounds, reps = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("REPS", 6))
    H, f, A, b0 = qpb.generate(n, B, 1, family="dense", m=m, shift=1.0, box=10.0, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    xc = (torch.rand((B, n), dtype=torch.float64, device=dev, generator=gen) - 0.5) * 0.2
    b = b0.clone()
    b[:, :meq] = torch.einsum("bij,bj->bi", A[:, :meq], xc)
    A2 = torch.cat([A, -A[:, :meq]], dim=1).contiguous()
    b2 = torch.cat([b, -b[:, :meq]], dim=1).contiguous()
    del xc
    legs = {
        "eq": lambda o: qpb.solve_eq(H, f, A, b, meq, out=o),
        "pairs": lambda o: qpb.solve(H, f, A2, b2, out=o),
        "plain": lambda o: qpb.solve(H, f, A, b0, out=o),
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
    res = {"n": n, "m": m, "meq": meq, "B": B, "rounds": rounds, "reps": reps, "library": qpb.version()[:8],
           "rows": {"eq": m, "pairs": m + meq, "plain": m}, "legs": {}}
    for nm in legs:
        t = sorted(times[nm])
        st = sols[nm].status
        res["legs"][nm] = {"median_ms": t[len(t) // 2], "min_ms": t[0], "round_medians_ms": rmed[nm],
                           "spread_ms": max(rmed[nm]) - min(rmed[nm]),
                           "status_counts": torch.bincount(st, minlength=5).tolist(),
                           "mean_iters": float(sols[nm].iters.double().mean())}
    xe, xp = sols["eq"].x, sols["pairs"].x
    ok = (sols["eq"].status == 0) & (sols["pairs"].status == 0)
    rel = (xe - xp).abs().amax(1) / xp.abs().amax(1).clamp(min=1.0)
    res["eq_vs_pairs_max_rel_x"] = float(rel[ok].max()) if bool(ok.any()) else None
    res["eq_over_pairs"] = res["legs"]["eq"]["median_ms"] / res["legs"]["pairs"]["median_ms"]
    res["eq_over_plain"] = res["legs"]["eq"]["median_ms"] / res["legs"]["plain"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
