#!/usr/bin/env python3
"""Timing of qpb_solve_backward on data generated on the device, against the
forward solve of the same batch, rounds interleaved as in tools/ab.py (clock
and thermal drift hit every leg alike):
  forward  qpb_solve                                   the yardstick of the same session
  all      qpb_solve_backward, gH gf gA gb             all four gradients
  fb       qpb_solve_backward, gf gb only              what a caller who learns f and b pays
  python tools/ab_backward.py N M B OUT.json
The QPs are qpb_generate's dense family; the backward is fed the forward's own
x, lam, active and status, and a seeded normal cotangent.
Per leg: the median and minimum over all launches, the median of each round
and their spread (max - min), the noise a difference has to clear.  The
backward legs are also set against their HBM floor: the bytes a QP must read
(H, A, x, lam, active, status, gx) and write (the gradients asked for) at
8 TB/s.  The gradients' certificate (the residuals of the backward system,
tests/kkt_oracle.py's, on the device) is reported for the first 4,096 QPs.
env: ROUNDS (5), REPS (6)"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "embedded-qp-solver_amd"))
import torch  # noqa: E402

import qpb  # noqa: E402

HBM_BYTES_PER_S = 8e12


def certificate(H, A, mask, g, gf, gb):
    """The two relative residuals of the backward system from the outputs (dx = gf, dlam = -gb on W)."""
    dl = torch.where(mask, -gb, torch.zeros_like(gb))
    r1 = torch.einsum("bij,bj->bi", H, gf) + torch.einsum("bij,bi->bj", A, dl) + g
    dxn = gf.abs().amax(1)
    stat = r1.abs().amax(1) / (1.0 + g.abs().amax(1) + H.abs().sum(2).amax(1) * dxn)
    r2 = torch.where(mask, torch.einsum("bij,bj->bi", A, gf), torch.zeros_like(gb))
    prim = r2.abs().amax(1) / (1.0 + A.abs().sum(2).amax(1) * dxn)
    return float(stat.max()), float(prim.max())


def main(n, m, B, out_path):
    dev = torch.device("cuda", 0)
    rounds, reps = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("REPS", 6))
    H, f, A, b = qpb.generate(n, B, 1, family="dense", m=m, shift=1.0, box=10.0, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    gx = torch.randn((B, n), dtype=torch.float64, device=dev, generator=gen)
    sol = qpb.solve(H, f, A, b)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
    gH, gf, gA, gb = new(B, n, n), new(B, n), new(B, m, n), new(B, m)
    d = qpb.Desc(n, m, B, 0, 0, 0.0)
    s = torch.cuda.current_stream()
    p = lambda t: qpb._ptr(t)  # noqa: E731

    def backward(oH, oA):
        rc = qpb.lib().qpb_solve_backward(ctypes.byref(d), p(H), p(A), p(sol.x), p(sol.lam), p(sol.active),
                                          p(sol.status), p(gx), p(oH), p(gf), p(oA), p(gb),
                                          ctypes.c_void_p(s.cuda_stream))
        assert rc == 0, qpb.lib().qpb_last_error()

    legs = {
        "forward": lambda: qpb.solve(H, f, A, b, out=sol),
        "all": lambda: backward(gH, gA),
        "fb": lambda: backward(None, None),
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
    w = (m + 31) // 32
    read = 8 * (n * n + m * n + n + m + n) + 4 * w + 4
    write = {"all": 8 * (n * n + n + m * n + m), "fb": 8 * (n + m)}
    res = {"n": n, "m": m, "B": B, "rounds": rounds, "reps": reps, "library": qpb.version()[:8],
           "status_counts": torch.bincount(sol.status, minlength=5).tolist(),
           "mean_active_rows": float(torch.from_numpy(qpb.active_mask_to_bool(sol.active[:4096].cpu().numpy(), m))
                                     .double().sum(1).mean()),
           "legs": {}}
    for nm in legs:
        t = sorted(times[nm])
        res["legs"][nm] = {"median_ms": t[len(t) // 2], "min_ms": t[0], "round_medians_ms": rmed[nm],
                           "spread_ms": max(rmed[nm]) - min(rmed[nm])}
    for nm in ("all", "fb"):
        leg = res["legs"][nm]
        leg["bytes_per_qp"] = {"read": read, "write": write[nm]}
        leg["hbm_floor_ms"] = (read + write[nm]) * B / HBM_BYTES_PER_S * 1e3
        leg["fraction_of_hbm_floor"] = leg["hbm_floor_ms"] / leg["median_ms"]
        leg["over_forward"] = leg["median_ms"] / res["legs"]["forward"]["median_ms"]
    k = slice(0, min(B, 4096))
    okq = sol.status[k] == 0
    mask = torch.from_numpy(qpb.active_mask_to_bool(sol.active[k].cpu().numpy(), m)).to(dev)
    stat, prim = certificate(H[k][okq], A[k][okq], mask[okq], gx[k][okq], gf[k][okq], gb[k][okq])
    res["certificate_first_4096"] = {"stat": stat, "prim": prim}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
