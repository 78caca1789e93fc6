#!/usr/bin/env python3
"""One H and one A for the whole batch: the new calls against what a caller had
to do before, rounds interleaved as in tools/ab_backward.py (clock and thermal
drift hit every leg alike):
  fwd_a   qpb_solve_eq on B materialised copies of H0 and A0
  bwd_a   qpb_solve_backward, all four gradients, on the copies, then the two
          sum(0) reductions that give dl/dH0 and dl/dA0
  fwd_b   qpb_solve_shared, shared = H | A, on the one copy
  bwd_b   qpb_solve_shared_backward, all four gradients (gH n x n, gA m x n)
  bwd_b1  ... gf and gb only: pass 1 alone, so bwd_b - bwd_b1 is the sum kernels'
  python tools/ab_shared.py N M B OUT.json
H0 and A0 are QP 0 of qpb_generate's dense family, f and b every QP's own
(b > 0: x = 0 is feasible for every QP).  Per leg: the median and minimum over
all launches, the median of each round and their spread (max - min), the noise
a difference has to clear.  The sum kernels are set against their HBM floor:
the bytes they read by shape (x, gf, gb, lam, active, status) at 8 TB/s.
Bytes allocated: the inputs and outputs of each leg by torch's accounting
(leg b's workspace, outside torch, is added by shape).
Checked at this size: fwd_b's outputs and bwd_b's gf and gb bitwise equal to leg
a's; gH and gA of leg b against leg a's sum(0) (torch's pairwise fp64 sum: its
own error is far below the bound) within (B + 4) 2^-53 T, T the sum of the
absolute values of the products; gH symmetric bit for bit.
env: ROUNDS (5), REPS (6) -- 30 launches per leg"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "embedded-qp-solver_amd"))
import torch  # noqa: E402

import qpb  # noqa: E402

HBM_BYTES_PER_S = 8e12


def main(n, m, B, out_path):
    dev = torch.device("cuda", 0)
    rounds, reps = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("REPS", 6))
    mem = lambda: torch.cuda.memory_allocated(dev)  # noqa: E731
    H, f, A, b = qpb.generate(n, B, 1, family="dense", m=m, shift=1.0, box=10.0, device=dev)
    H0, A0 = H[0].clone(), A[0].clone()
    del H, A
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    gx = torch.randn((B, n), dtype=torch.float64, device=dev, generator=gen)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
    m0 = mem()
    # leg a: the copies and the per-QP gradients
    Hc, Ac = H0.expand(B, n, n).contiguous(), A0.expand(B, m, n).contiguous()
    sol_a = qpb.solve_eq(Hc, f, Ac, b, 0)
    gHa, gfa, gAa, gba = new(B, n, n), new(B, n), new(B, m, n), new(B, m)
    bytes_a = mem() - m0
    m1 = mem()
    sol_b = qpb.solve_shared(H0, f, A0, b, 0)
    gHb, gfb, gAb, gbb = new(n, n), new(B, n), new(m, n), new(B, m)
    bytes_b = mem() - m1
    slots, _ = qpb.sum_plan(B)
    ws_b = slots * 256 * ((n + 15) // 16) * ((n + 15) // 16 + (m + 15) // 16) * 8
    s = torch.cuda.current_stream()
    sp = ctypes.c_void_p(s.cuda_stream)
    p = lambda t: qpb._ptr(t)  # noqa: E731
    d = qpb.Desc(n, m, B, 0, 0, 0.0)
    sums = {}

    def bwd_a():
        rc = qpb.lib().qpb_solve_backward(ctypes.byref(d), p(Hc), p(Ac), p(sol_a.x), p(sol_a.lam), p(sol_a.active),
                                          p(sol_a.status), p(gx), p(gHa), p(gfa), p(gAa), p(gba), sp)
        assert rc == 0, qpb.lib().qpb_last_error()
        sums["H"], sums["A"] = gHa.sum(0), gAa.sum(0)

    def bwd_b(oH, oA):
        rc = qpb.lib().qpb_solve_shared_backward(ctypes.byref(d), 3, p(H0), p(A0), p(sol_b.x), p(sol_b.lam),
                                                 p(sol_b.active), p(sol_b.status), p(gx), p(oH), p(gfb), p(oA),
                                                 p(gbb), sp)
        assert rc == 0, qpb.lib().qpb_last_error()

    legs = {
        "fwd_a": lambda: qpb.solve_eq(Hc, f, Ac, b, 0, out=sol_a),
        "fwd_b": lambda: qpb.solve_shared(H0, f, A0, b, 0, out=sol_b),
        "bwd_a": bwd_a,
        "bwd_b": lambda: bwd_b(gHb, gAb),
        "bwd_b1": lambda: bwd_b(None, None),
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
                fn()
                e1.record(s)
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            times[nm] += ts
            rmed[nm].append(sorted(ts)[len(ts) // 2])
    res = {"n": n, "m": m, "B": B, "rounds": rounds, "reps": reps, "library": qpb.version()[:8],
           "status_counts": torch.bincount(sol_b.status, minlength=5).tolist(), "sum_slots": slots,
           "bytes_allocated": {"a": bytes_a, "b": bytes_b, "b_workspace_by_shape": ws_b}, "legs": {}}
    for nm in legs:
        t = sorted(times[nm])
        res["legs"][nm] = {"median_ms": t[len(t) // 2], "min_ms": t[0], "round_medians_ms": rmed[nm],
                           "spread_ms": max(rmed[nm]) - min(rmed[nm])}
    L = res["legs"]
    w = (m + 31) // 32
    sum_read = B * (8 * (2 * n + 2 * m) + 4 * w + 4)
    sum_ms = L["bwd_b"]["median_ms"] - L["bwd_b1"]["median_ms"]
    res["sum_kernels"] = {"ms_bwd_b_minus_bwd_b1": sum_ms, "bytes_read_by_shape": sum_read,
                          "hbm_floor_ms": sum_read / HBM_BYTES_PER_S * 1e3}
    res["forward_b_minus_a_ms"] = L["fwd_b"]["median_ms"] - L["fwd_a"]["median_ms"]
    res["backward_a_minus_b_ms"] = L["bwd_a"]["median_ms"] - L["bwd_b"]["median_ms"]
    res["backward_gain_over_3_spreads_of_a"] = res["backward_a_minus_b_ms"] / (3 * L["bwd_a"]["spread_ms"]) \
        if L["bwd_a"]["spread_ms"] > 0 else None
    # ---- the outputs at this size
    legs["bwd_a"]()
    legs["bwd_b"]()
    torch.cuda.synchronize()
    eq = lambda a, c: bool(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,  # noqa: E731
                                       c.view(torch.int64) if c.dtype == torch.float64 else c))
    ok = sol_b.status == 0
    x = torch.where(ok[:, None], sol_b.x, torch.zeros_like(sol_b.x)).abs()
    dx, dl = gfb.abs(), gbb.abs()
    mask = torch.from_numpy(qpb.active_mask_to_bool(sol_b.active.cpu().numpy(), m)).to(dev)
    lm = torch.where(mask & ok[:, None], sol_b.lam, torch.zeros_like(sol_b.lam)).abs()
    u = (B + 4) * 2.0 ** -53
    bH = u * 0.5 * (dx.T @ x + x.T @ dx)
    bA = u * (dl.T @ x + lm.T @ dx)
    ratio = lambda got, want, bound: float(torch.where(bound > 0, (got - want).abs() / bound,  # noqa: E731
                                                       (got - want).abs() * float("inf")).nan_to_num(0.0).max())
    res["checks"] = {
        "forward_bitwise": all(eq(getattr(sol_a, k), getattr(sol_b, k))
                               for k in ("x", "lam", "active", "status", "iters")),
        "gf_gb_bitwise": eq(gfa, gfb) and eq(gba, gbb),
        "gH_symmetric_bitwise": eq(gHb, gHb.T.contiguous()),
        "gH_worst_delta_over_bound": ratio(gHb, sums["H"], bH),
        "gA_worst_delta_over_bound": ratio(gAb, sums["A"], bA),
    }
    c = res["checks"]
    res["checks"]["pass"] = bool(c["forward_bitwise"] and c["gf_gb_bitwise"] and c["gH_symmetric_bitwise"]
                                 and c["gH_worst_delta_over_bound"] <= 1.0 and c["gA_worst_delta_over_bound"] <= 1.0)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
