#!/usr/bin/env python3
"""Timing of qpb_solve_box_backward on data generated on the device, against
the forward box solve of the same batch and against what a caller could do
before the call existed, rounds interleaved as in tools/ab_backward.py (clock
and thermal drift hit every leg alike):
  forward  qpb_solve_box                                    (a) the yardstick of the same session
  general  qpb_solve_backward, explicit A = [I; -I],        (b) gH gf gb (gA NULL)
  box      qpb_solve_box_backward, gH gf glb gub            (c)
  python tools/ab_box_backward.py N B OUT.json
The QPs are qpb_generate's box family (its A and b are the explicit rows: ub =
b[:n], lb = -b[n:]); both backward legs are fed the forward's own x, lam,
active and status, and a seeded normal cotangent.
Per leg: the median and minimum over all launches, the median of each round
and their spread (max - min), the noise a difference has to clear.  The
backward legs are also set against their HBM floors: the bytes a QP must read
and write at 8 TB/s (box: H, x, gx, the mask words and status in; gH, gf, glb,
gub out: 4,744 B at n = 16).  The two backward legs' outputs are compared
(bwd_harness.rel's measure over the whole batch) and the box leg's
certificate on the explicit A is reported for the first 4,096 QPs.
env: ROUNDS (5), REPS (6): 30 launches per leg"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "embedded-qp-solver_amd"))
import torch  # noqa: E402

import qpb  # noqa: E402

HBM_BYTES_PER_S = 8e12


def rel(a, ref):
    """max over the batch of max|delta| / (1 + max|ref|) per QP."""
    a, ref = a.reshape(len(a), -1), ref.reshape(len(ref), -1)
    return float(((a - ref).abs().amax(1) / (1.0 + ref.abs().amax(1))).max())


def certificate(H, up, lo, g, gf, glb, gub):
    """The residuals of the backward system on the explicit A from the outputs:
    dx = gf, A_W^T dlam = -(gub + glb) (at most one of the two is nonzero)."""
    r1 = torch.einsum("bij,bj->bi", H, gf) - (gub + glb) + g
    dxn = gf.abs().amax(1)
    stat = r1.abs().amax(1) / (1.0 + g.abs().amax(1) + H.abs().sum(2).amax(1) * dxn)
    prim = torch.where(up | lo, gf, torch.zeros_like(gf)).abs().amax(1) / (1.0 + dxn)
    return float(stat.max()), float(prim.max())


def main(n, B, out_path):
    dev = torch.device("cuda", 0)
    rounds, reps = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("REPS", 6))
    m = 2 * n
    H, f, A, b = qpb.generate(n, B, 1, family="box", device=dev)
    ub, lb = b[:, :n].contiguous(), (-b[:, n:]).contiguous()
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    gx = torch.randn((B, n), dtype=torch.float64, device=dev, generator=gen)
    sol = qpb.solve_box(H, f, lb, ub)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
    gH, gf, gb = new(B, n, n), new(B, n), new(B, m)
    bH, bf, bl, bu = new(B, n, n), new(B, n), new(B, n), new(B, n)
    d = qpb.Desc(n, m, B, 0, 0, 0.0)
    s = torch.cuda.current_stream()
    p = lambda t: qpb._ptr(t)  # noqa: E731

    def general():
        rc = qpb.lib().qpb_solve_backward(ctypes.byref(d), p(H), p(A), p(sol.x), p(sol.lam), p(sol.active),
                                          p(sol.status), p(gx), p(gH), p(gf), None, p(gb),
                                          ctypes.c_void_p(s.cuda_stream))
        assert rc == 0, qpb.lib().qpb_last_error()

    def box():
        rc = qpb.lib().qpb_solve_box_backward(ctypes.byref(d), p(H), p(sol.x), p(sol.active), p(sol.status), p(gx),
                                              p(bH), p(bf), p(bl), p(bu), ctypes.c_void_p(s.cuda_stream))
        assert rc == 0, qpb.lib().qpb_last_error()

    legs = {
        "forward": lambda: qpb.solve_box(H, f, lb, ub, out=sol),
        "general": general,
        "box": box,
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
    traffic = {
        "general": {"read": 8 * (n * n + m * n + n + m + n) + 4 * w + 4, "write": 8 * (n * n + n + m)},
        "box": {"read": 8 * (n * n + n + n) + 4 * w + 4, "write": 8 * (n * n + 3 * n)},
    }
    mask = torch.from_numpy(qpb.active_mask_to_bool(sol.active[:4096].cpu().numpy(), m)).to(dev)
    res = {"n": n, "m": m, "B": B, "rounds": rounds, "reps": reps, "library": qpb.version()[:8],
           "status_counts": torch.bincount(sol.status, minlength=5).tolist(),
           "mean_active_rows": float(mask.double().sum(1).mean()), "legs": {}}
    for nm in legs:
        t = sorted(times[nm])
        res["legs"][nm] = {"median_ms": t[len(t) // 2], "min_ms": t[0], "round_medians_ms": rmed[nm],
                           "spread_ms": max(rmed[nm]) - min(rmed[nm])}
    for nm in ("general", "box"):
        leg = res["legs"][nm]
        leg["bytes_per_qp"] = traffic[nm]
        leg["hbm_floor_ms"] = (traffic[nm]["read"] + traffic[nm]["write"]) * B / HBM_BYTES_PER_S * 1e3
        leg["fraction_of_hbm_floor"] = leg["hbm_floor_ms"] / leg["median_ms"]
        leg["over_forward"] = leg["median_ms"] / res["legs"]["forward"]["median_ms"]
    gl, bx = res["legs"]["general"], res["legs"]["box"]
    bx["over_general"] = bx["median_ms"] / gl["median_ms"]
    # the claim: the box leg beats the general one by more than the general leg's spread of round medians
    res["box_beats_general_by_more_than_its_spread"] = bool(gl["median_ms"] - bx["median_ms"] > gl["spread_ms"])
    res["box_against_general"] = {"gH": rel(bH, gH), "gf": rel(bf, gf), "gub": rel(bu, gb[:, :n]),
                                  "glb": rel(bl, -gb[:, n:])}
    k = slice(0, min(B, 4096))
    okq = sol.status[k] == 0
    up, lo = mask[:, :n][okq], mask[:, n:][okq]
    stat, prim = certificate(H[k][okq], up, lo, gx[k][okq], bf[k][okq], bl[k][okq], bu[k][okq])
    res["certificate_first_4096"] = {"stat": stat, "prim": prim}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3])
