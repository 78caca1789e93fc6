#!/usr/bin/env python3
"""What a cotangent on lam costs: qpb_solve_backward_dual against
qpb_solve_backward on data generated on the device, rounds interleaved as in
tools/ab_backward.py (clock and thermal drift hit every leg alike):
  a    qpb_solve_backward, all four gradients -- on the library PARENT_LIB names
       (the build of the commit before), else on this one
  b    qpb_solve_backward_dual with glam = NULL: must be a's kernels
  c    qpb_solve_backward_dual with a seeded normal glam: the DU forms
  a1, b1, c1   the same with gf and gb only (no gH / gA stores: the solve itself)
  python tools/ab_backward_dual.py N M B OUT.json
The QPs are qpb_generate's dense family; the backward is fed the forward's own
x, lam, active and status and a seeded normal gx.  Per leg: the median and
minimum over all launches, the median of each round and their spread
(max - min).  b - a and c - a are reported against three spreads of a's round
medians, whichever way they fall.  Checked at this size: b's outputs equal a's
bit for bit; c's certificate (the two residuals of the system with glam_W, on
the device) for the first 4,096 QPs.
env: ROUNDS (5), REPS (6) -- 30 timed launches per leg; PARENT_LIB"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "embedded-qp-solver_amd"))
import torch  # noqa: E402

import qpb  # noqa: E402


def certificate(H, A, mask, g, gl, gf, gb):
    """The two relative residuals of the system from the outputs (dx = gf, dlam = -gb on W)."""
    zero = torch.zeros_like(gb)
    dl = torch.where(mask, -gb, zero)
    glw = torch.where(mask, gl, zero)
    r1 = torch.einsum("bij,bj->bi", H, gf) + torch.einsum("bij,bi->bj", A, dl) + g
    dxn = gf.abs().amax(1)
    stat = r1.abs().amax(1) / (1.0 + g.abs().amax(1) + H.abs().sum(2).amax(1) * dxn)
    r2 = torch.where(mask, torch.einsum("bij,bj->bi", A, gf) + gl, zero)
    prim = r2.abs().amax(1) / (1.0 + glw.abs().amax(1) + A.abs().sum(2).amax(1) * dxn)
    return float(stat.max()), float(prim.max())


def main(n, m, B, out_path):
    dev = torch.device("cuda", 0)
    rounds, reps = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("REPS", 6))
    parent_path = os.environ.get("PARENT_LIB")
    parent = ctypes.CDLL(parent_path) if parent_path else qpb.lib()
    vp = ctypes.c_void_p
    parent.qpb_solve_backward.argtypes = [ctypes.POINTER(qpb.Desc)] + [vp] * 12
    parent.qpb_solve_backward.restype = ctypes.c_int
    H, f, A, b = qpb.generate(n, B, 1, family="dense", m=m, shift=1.0, box=10.0, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    gx = torch.randn((B, n), dtype=torch.float64, device=dev, generator=gen)
    gl = torch.randn((B, m), dtype=torch.float64, device=dev, generator=gen)
    sol = qpb.solve(H, f, A, b)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
    outs = {nm: (new(B, n, n), new(B, n), new(B, m, n), new(B, m)) for nm in "abc"}
    d = qpb.Desc(n, m, B, 0, 0, 0.0)
    s = torch.cuda.current_stream()
    p = lambda t: qpb._ptr(t)  # noqa: E731
    ins = lambda: (p(H), p(A), p(sol.x), p(sol.lam), p(sol.active), p(sol.status), p(gx))  # noqa: E731

    def plain(o, full):
        gH, gf, gA, gb = o
        rc = parent.qpb_solve_backward(ctypes.byref(d), *ins(), p(gH if full else None), p(gf),
                                       p(gA if full else None), p(gb), vp(s.cuda_stream))
        assert rc == 0

    def dual(o, glam, full):
        gH, gf, gA, gb = o
        rc = qpb.lib().qpb_solve_backward_dual(ctypes.byref(d), 0, *ins(), p(glam), p(gH if full else None), p(gf),
                                               p(gA if full else None), p(gb), vp(s.cuda_stream))
        assert rc == 0, qpb.lib().qpb_last_error()

    legs = {
        "a": lambda: plain(outs["a"], True),
        "b": lambda: dual(outs["b"], None, True),
        "c": lambda: dual(outs["c"], gl, True),
        "a1": lambda: plain(outs["a"], False),
        "b1": lambda: dual(outs["b"], None, False),
        "c1": lambda: dual(outs["c"], gl, False),
    }
    for fn in legs.values():
        for _ in range(3):
            fn()
    for nm in "abc":  # the full legs last: what the checks read
        legs[nm]()
    torch.cuda.synchronize()
    same = lambda u, v: bool(torch.equal(u.view(torch.int64), v.view(torch.int64)))  # noqa: E731
    checks = {"b_bitwise_a": all(same(u, v) for u, v in zip(outs["b"], outs["a"])),
              "c_finite": bool(all(torch.isfinite(t).all() for t in outs["c"]))}
    k = slice(0, min(B, 4096))
    okq = sol.status[k] == 0
    mask = torch.from_numpy(qpb.active_mask_to_bool(sol.active[k].cpu().numpy(), m)).to(dev)
    stat, prim = certificate(H[k][okq], A[k][okq], mask[okq], gx[k][okq], gl[k][okq], outs["c"][1][k][okq],
                             outs["c"][3][k][okq])
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
           "leg_a_library": parent_path or "this one",
           "status_counts": torch.bincount(sol.status, minlength=5).tolist(),
           "mean_active_rows": float(mask.double().sum(1).mean()), "legs": {}}
    for nm in legs:
        t = sorted(times[nm])
        res["legs"][nm] = {"median_ms": t[len(t) // 2], "min_ms": t[0], "round_medians_ms": rmed[nm],
                           "spread_ms": max(rmed[nm]) - min(rmed[nm])}
    L = res["legs"]
    for x, a in (("b", "a"), ("c", "a"), ("b1", "a1"), ("c1", "a1")):
        diff = L[x]["median_ms"] - L[a]["median_ms"]
        bar = 3 * L[a]["spread_ms"]
        res[f"{x}_minus_{a}"] = {"ms": diff, "ratio": L[x]["median_ms"] / L[a]["median_ms"],
                                 "bar_ms_3_spreads_of_" + a: bar, "beyond_bar": bool(abs(diff) > bar)}
    res["checks"] = checks
    res["certificate_c_first_4096"] = {"stat": stat, "prim": prim}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
