#!/usr/bin/env python3
"""Timing of qpb_solve_range_box against the call it replaces, qpb_solve_range on
a materialised A' = [G; I], on the same QPs, rounds interleaved as in
tools/ab_range.py (clock and thermal drift hit every leg alike):
  mat      qpb_solve_range(A', [bl; lb], [bu; ub])   A' built beforehand
  mat_cat  the same with the torch.cat that builds A' inside the timed region
  box      qpb_solve_range_box(G, bl, bu, lb, ub)    no A' anywhere
  python tools/ab_range_box.py N MG B OUT.json
The QPs are the test family (tests/range_box_oracle.py: range_family's rows,
strictly feasible at xc, and a box around xc that binds) scaled up: BASE QPs
are generated, and the batch draws B of them independently and uniformly
(seeded), every QP with its own copy of every array, so neighbouring QPs in a
wavefront differ as they do in the family.
Per leg: the median and minimum over all launches, the median of each round
and their spread (max - min), the noise a difference has to clear: a
difference counts when it exceeds three times the spread of the mat leg.
The outputs of box are compared with mat's, all six, bit for bit; the bytes
each leg needs beside H, f and the bounds are recorded.
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


def main(n, mg, B, out_path):
    dev = torch.device("cuda", 0)
    rounds, reps = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("REPS", 6))
    base = min(int(os.environ.get("BASE", 4096)), B)
    fam = BO.box_family(base, n, mg, 0)[:7]
    idx = torch.from_numpy(np.random.default_rng([n, mg, B]).integers(0, base, size=B)).to(dev)
    H, f, G, bl, bu, lb, ub = (torch.from_numpy(np.ascontiguousarray(v)).to(dev)[idx].contiguous() for v in fam)
    eye = torch.eye(n, dtype=torch.float64, device=dev)
    Ap = torch.cat([G, eye.expand(B, n, n)], dim=1).contiguous()
    lo = torch.cat([bl, lb], dim=1).contiguous()
    hi = torch.cat([bu, ub], dim=1).contiguous()
    Gn = G if mg else None
    legs = {
        "mat": lambda o: qpb.solve_range(H, f, Ap, lo, hi, out=o),
        "mat_cat": lambda o: qpb.solve_range(H, f, torch.cat([G, eye.expand(B, n, n)], dim=1), lo, hi, out=o),
        "box": lambda o: qpb.solve_range_box(H, f, Gn, bl if mg else None, bu if mg else None, lb, ub, out=o),
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
    a_bytes = B * (mg + n) * n * 8
    res = {"n": n, "mg": mg, "rows": mg + n, "B": B, "base": base, "rounds": rounds, "reps": reps,
           "library": qpb.version()[:8],
           "input_bytes_per_qp": {"mat": 8 * (n * n + n + (mg + n) * n + 2 * (mg + n)),
                                  "box": 8 * (n * n + n + mg * n + 2 * (mg + n))},
           "bytes_allocated_for_A": {"mat": a_bytes, "mat_cat": a_bytes, "box": 0},
           "A_is_built": {"mat": "once, before the timing", "mat_cat": "per call, inside the timing", "box": "never"},
           "legs": {}}
    for nm in legs:
        t = sorted(times[nm])
        st = sols[nm].status
        res["legs"][nm] = {"median_ms": t[len(t) // 2], "min_ms": t[0], "round_medians_ms": rmed[nm],
                           "spread_ms": max(rmed[nm]) - min(rmed[nm]),
                           "status_counts": torch.bincount(st, minlength=5).tolist(),
                           "mean_iters": float(sols[nm].iters.double().mean())}
    rows = torch.arange(mg + n, device=dev)
    bits = lambda words: ((words[:, rows // 32] >> (rows % 32)) & 1)  # noqa: E731
    act, low = bits(sols["box"].active), bits(sols["box"].lower)
    res["box_active_per_qp"] = {"rows_upper": float((act & ~low)[:, :mg].sum()) / B, "rows_lower": float(low[:, :mg].sum()) / B,
                                "bounds_upper": float((act & ~low)[:, mg:].sum()) / B,
                                "bounds_lower": float(low[:, mg:].sum()) / B}
    raw = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t  # noqa: E731
    same = lambda p, q: all(torch.equal(raw(u), raw(v)) for u, v in zip(p, q))  # noqa: E731
    res["box_equals_mat_bit_for_bit"] = same(sols["box"], sols["mat"])
    res["mat_cat_equals_mat_bit_for_bit"] = same(sols["mat_cat"], sols["mat"])
    res["all_ok"] = bool((sols["box"].status == 0).all())
    med = {nm: res["legs"][nm]["median_ms"] for nm in legs}
    margin = 3.0 * res["legs"]["mat"]["spread_ms"]
    res["box_minus_mat_ms"] = med["box"] - med["mat"]
    res["box_minus_mat_cat_ms"] = med["box"] - med["mat_cat"]
    res["box_over_mat"] = med["box"] / med["mat"]
    res["box_over_mat_cat"] = med["box"] / med["mat_cat"]
    res["three_spreads_of_mat_ms"] = margin
    res["box_not_slower"] = med["box"] - med["mat"] < margin  # the requirement
    res["gain_clears_three_spreads"] = med["mat"] - med["box"] > margin
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    if not res["box_equals_mat_bit_for_bit"]:
        sys.exit("the outputs of qpb_solve_range_box differ from qpb_solve_range's on the materialised problem")


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
