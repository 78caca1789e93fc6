#!/usr/bin/env python3
"""Timing of qpb_solve_range_box_backward against what it replaces, the backward
on a materialised A' = [G; I] as qpb.diff.solve_range_box ran it before, on the
same solved QPs, rounds interleaved as in tools/ab_range_box.py (clock and
thermal drift hit every leg alike):
  mat      qpb_solve_backward(A')   A' built beforehand, then the slice of gA' and
           the four-way routing of gb' by the `lower` bits (torch.where)
  mat_cat  the same with the torch.cat that builds A' inside the timed region:
           what a training step paid
  box      qpb_solve_range_box_backward(G)   no A', no gA', no routing pass
  python tools/ab_range_box_backward.py N MG B OUT.json
Each leg is timed twice: with all seven gradients ("all") and with need =
(f, bl, bu, lb, ub) only ("f_bounds": no matrix output).
The QPs are tools/ab_range_box.py's (tests/range_box_oracle.py's family, BASE
QPs drawn B times), solved once by qpb_solve_range_box; gx is a seeded normal.
Per leg: the median and minimum over all launches, the median of each round
and their spread (max - min), the noise a difference has to clear: a
difference counts when it exceeds three times the spread of the mat leg.
The outputs of box are compared with mat's, all seven, bit for bit; the peak
bytes each leg allocates during one call are recorded.
env: ROUNDS (5), REPS (6), BASE (4096)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "embedded-qp-solver_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import qpb  # noqa: E402
import range_box_oracle as BO  # noqa: E402

NEEDS = {"all": ("H", "f", "G", "bl", "bu", "lb", "ub"), "f_bounds": ("f", "bl", "bu", "lb", "ub")}


def main(n, mg, B, out_path):
    dev = torch.device("cuda", 0)
    rounds, reps = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("REPS", 6))
    base = min(int(os.environ.get("BASE", 4096)), B)
    fam = BO.box_family(base, n, mg, 0)[:7]
    idx = torch.from_numpy(np.random.default_rng([n, mg, B]).integers(0, base, size=B)).to(dev)
    H, f, G, bl, bu, lb, ub = (torch.from_numpy(np.ascontiguousarray(v)).to(dev)[idx].contiguous() for v in fam)
    rsol = qpb.solve_range_box(H, f, G, bl, bu, lb, ub)
    del f, bl, bu, lb, ub
    sol = qpb.Solution(rsol.x, rsol.lam, rsol.active, rsol.status, None)
    gx = torch.from_numpy(np.random.default_rng([n, mg, B, 1]).standard_normal((B, n))).to(dev)
    eye = torch.eye(n, dtype=torch.float64, device=dev)
    rows = torch.arange(mg + n, device=dev)

    def mat(need, Ap):
        # qpb.diff.RangeBoxQPFunction.backward as it was: the call, the slice, the routing
        want = [k for k in "Hf" if k in need] + (["A"] if "G" in need else []) + ["b"]
        gH, gf, gA, gb = qpb.solve_backward(H, Ap, sol, gx, need=want)
        gG = None if gA is None else gA[..., :mg, :]
        low = ((rsol.lower[:, rows // 32] >> (rows % 32)) & 1).bool()
        zero = torch.zeros_like(gb)
        to_lo, to_hi = torch.where(low, gb, zero), torch.where(low, zero, gb)
        return gH, gf, gG, to_lo[:, :mg], to_hi[:, :mg], to_lo[:, mg:], to_hi[:, mg:]

    res = {"n": n, "mg": mg, "rows": mg + n, "B": B, "base": base, "rounds": rounds, "reps": reps,
           "library": qpb.version()[:8], "all_ok": bool((rsol.status == 0).all()),
           "A_is_built": {"mat": "once, before the timing", "mat_cat": "per call, inside the timing", "box": "never"},
           "needs": {}}
    s = torch.cuda.current_stream()
    for tag, need in NEEDS.items():
        Ap = torch.cat([G, eye.expand(B, n, n)], dim=1).contiguous()
        legs = {
            "mat": lambda: mat(need, Ap),
            "mat_cat": lambda: mat(need, torch.cat([G, eye.expand(B, n, n)], dim=1)),
            "box": lambda: qpb.solve_range_box_backward(H, G, rsol, gx, need=need),
        }
        outs, peak = {}, {}
        for nm, fn in legs.items():
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            outs[nm] = fn()
            torch.cuda.synchronize()
            peak[nm] = torch.cuda.max_memory_allocated() - before
        raw = lambda t: t.contiguous().view(torch.int64)  # noqa: E731
        same = all((p is None and q is None) or torch.equal(raw(p), raw(q)) for p, q in zip(outs["box"], outs["mat"]))
        del outs
        times = {nm: [] for nm in legs}
        rmed = {nm: [] for nm in legs}
        for _ in range(rounds):
            for nm, fn in legs.items():
                ts = []
                for _ in range(reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    fn()
                    e1.record(s)
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1))
                times[nm] += ts
                rmed[nm].append(sorted(ts)[len(ts) // 2])
        r = {"need": list(need), "box_equals_mat_bit_for_bit": bool(same),
             "peak_bytes_allocated_by_one_call": peak, "bytes_of_A": B * (mg + n) * n * 8, "legs": {}}
        for nm in legs:
            t = sorted(times[nm])
            r["legs"][nm] = {"median_ms": t[len(t) // 2], "min_ms": t[0], "round_medians_ms": rmed[nm],
                             "spread_ms": max(rmed[nm]) - min(rmed[nm])}
        med = {nm: r["legs"][nm]["median_ms"] for nm in legs}
        margin = 3.0 * r["legs"]["mat"]["spread_ms"]
        r["three_spreads_of_mat_ms"] = margin
        r["box_minus_mat_ms"] = med["box"] - med["mat"]
        r["box_minus_mat_cat_ms"] = med["box"] - med["mat_cat"]
        r["box_over_mat"] = med["box"] / med["mat"]
        r["box_over_mat_cat"] = med["box"] / med["mat_cat"]
        r["box_not_slower"] = med["box"] - med["mat"] < margin  # the requirement
        r["gain_over_mat_clears_three_spreads"] = med["mat"] - med["box"] > margin
        r["gain_over_mat_cat_clears_three_spreads"] = med["mat_cat"] - med["box"] > margin
        res["needs"][tag] = r
        del Ap, legs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    if not all(r["box_equals_mat_bit_for_bit"] for r in res["needs"].values()):
        sys.exit("the outputs of qpb_solve_range_box_backward differ from the materialised backward's")


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
