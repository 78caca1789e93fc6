#!/usr/bin/env python3
"""One H for a batch of box QPs: the new calls against what a caller had to do
before, rounds interleaved as in tools/ab_shared.py and tools/ab_box_backward.py
(clock and thermal drift hit every leg alike):
  fwd_a   qpb_solve_box on B materialised copies of H0
  bwd_a   qpb_solve_box_backward, all four gradients, on the copies, then
          gH.sum(0), which gives dl/dH0
  fwd_b   qpb_solve_box_shared on the one copy
  bwd_b   qpb_solve_box_shared_backward, all four gradients (gH n x n)
  bwd_b1  ... gf, glb and gub only: pass 1 alone, so bwd_b - bwd_b1 is the sum kernels'
  python tools/ab_box_shared.py N B OUT.json
Above n = 32 (no box backward) the forward legs alone run.
H0 is QP 0 of qpb_generate's box family, f, lb and ub every QP's own (its A and
b are the explicit rows: ub = b[:n], lb = -b[n:]).  Per leg: the median and
minimum over all launches, the median of each round and their spread
(max - min), the noise a difference has to clear: (a) - (b) is set against three
spreads of leg (a)'s round medians.
Bytes allocated: the inputs and outputs of each leg by torch's accounting (leg
b's workspace, outside torch, is added by shape).
Checked at this size: fwd_b's outputs and bwd_b's gf, glb and gub bitwise equal
to leg a's; gH of leg b against leg a's sum(0) (torch's pairwise fp64 sum: its
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


def main(n, B, out_path):
    dev = torch.device("cuda", 0)
    rounds, reps = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("REPS", 6))
    m = 2 * n
    with_bwd = n <= 32
    mem = lambda: torch.cuda.memory_allocated(dev)  # noqa: E731
    H, f, _, b = qpb.generate(n, B, 1, family="box", device=dev)
    ub, lb = b[:, :n].contiguous(), (-b[:, n:]).contiguous()
    H0 = H[0].clone()
    del H, b
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    gx = torch.randn((B, n), dtype=torch.float64, device=dev, generator=gen)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev) if with_bwd else None  # noqa: E731
    m0 = mem()
    # leg a: the copies and the per-QP gradient
    Hc = H0.expand(B, n, n).contiguous()
    sol_a = qpb.solve_box(Hc, f, lb, ub)
    gHa, gfa, gla, gua = new(B, n, n), new(B, n), new(B, n), new(B, n)
    bytes_a = mem() - m0
    m1 = mem()
    sol_b = qpb.solve_box_shared(H0, f, lb, ub)
    gHb, gfb, glb_, gub_ = new(n, n), new(B, n), new(B, n), new(B, n)
    bytes_b = mem() - m1
    slots, _ = qpb.sum_plan(B)
    ws_b = slots * 256 * ((n + 15) // 16) ** 2 * 8 if with_bwd else 0
    s = torch.cuda.current_stream()
    sp = ctypes.c_void_p(s.cuda_stream)
    p = lambda t: qpb._ptr(t)  # noqa: E731
    d = qpb.Desc(n, m, B, 0, 0, 0.0)
    sums = {}

    def bwd_a():
        rc = qpb.lib().qpb_solve_box_backward(ctypes.byref(d), p(Hc), p(sol_a.x), p(sol_a.active), p(sol_a.status),
                                              p(gx), p(gHa), p(gfa), p(gla), p(gua), sp)
        assert rc == 0, qpb.lib().qpb_last_error()
        sums["H"] = gHa.sum(0)

    def bwd_b(oH):
        rc = qpb.lib().qpb_solve_box_shared_backward(ctypes.byref(d), p(H0), p(sol_b.x), p(sol_b.active),
                                                     p(sol_b.status), p(gx), p(oH), p(gfb), p(glb_), p(gub_), sp)
        assert rc == 0, qpb.lib().qpb_last_error()

    legs = {
        "fwd_a": lambda: qpb.solve_box(Hc, f, lb, ub, out=sol_a),
        "fwd_b": lambda: qpb.solve_box_shared(H0, f, lb, ub, out=sol_b),
    }
    if with_bwd:
        legs.update({"bwd_a": bwd_a, "bwd_b": lambda: bwd_b(gHb), "bwd_b1": lambda: bwd_b(None)})
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
    res = {"n": n, "B": B, "rounds": rounds, "reps": reps, "library": qpb.version()[:8],
           "status_counts": torch.bincount(sol_b.status, minlength=5).tolist(), "sum_slots": slots,
           "bytes_allocated": {"a": bytes_a, "b": bytes_b, "b_workspace_by_shape": ws_b}, "legs": {}}
    for nm in legs:
        t = sorted(times[nm])
        res["legs"][nm] = {"median_ms": t[len(t) // 2], "min_ms": t[0], "round_medians_ms": rmed[nm],
                           "spread_ms": max(rmed[nm]) - min(rmed[nm])}
    L = res["legs"]

    def verdict(a, bb):
        gain, bar = L[a]["median_ms"] - L[bb]["median_ms"], 3 * L[a]["spread_ms"]
        return {"a_minus_b_ms": gain, "three_spreads_of_a_ms": bar, "relative": gain / L[a]["median_ms"],
                "verdict": "clears" if gain > bar else "does not clear"}

    res["forward"] = verdict("fwd_a", "fwd_b")
    eq = lambda a, c: bool(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,  # noqa: E731
                                       c.view(torch.int64) if c.dtype == torch.float64 else c))
    res["checks"] = {"forward_bitwise": all(eq(getattr(sol_a, k), getattr(sol_b, k))
                                            for k in ("x", "lam", "active", "status", "iters"))}
    c = res["checks"]
    c["pass"] = c["forward_bitwise"]
    if with_bwd:
        res["backward"] = verdict("bwd_a", "bwd_b")
        res["sum_kernels_ms_bwd_b_minus_bwd_b1"] = L["bwd_b"]["median_ms"] - L["bwd_b1"]["median_ms"]
        legs["bwd_a"]()
        legs["bwd_b"]()
        torch.cuda.synchronize()
        ok = sol_b.status == 0
        x = torch.where(ok[:, None], sol_b.x, torch.zeros_like(sol_b.x)).abs()
        dx = gfb.abs()
        bH = (B + 4) * 2.0 ** -53 * 0.5 * (dx.T @ x + x.T @ dx)
        delta = (gHb - sums["H"]).abs()
        c["gf_glb_gub_bitwise"] = eq(gfa, gfb) and eq(gla, glb_) and eq(gua, gub_)
        c["gH_symmetric_bitwise"] = eq(gHb, gHb.T.contiguous())
        c["gH_worst_delta_over_bound"] = float(torch.where(bH > 0, delta / bH, delta * float("inf"))
                                               .nan_to_num(0.0).max())
        c["pass"] = bool(c["forward_bitwise"] and c["gf_glb_gub_bitwise"] and c["gH_symmetric_bitwise"]
                         and c["gH_worst_delta_over_bound"] <= 1.0)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3])
