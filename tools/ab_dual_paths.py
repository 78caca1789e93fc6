#!/usr/bin/env python3
"""What glam costs on the two paths the library is built around, on data
generated on the device, rounds interleaved as in tools/ab_backward_dual.py and
tools/ab_box_backward.py (clock and thermal drift hit every leg alike).

  python tools/ab_dual_paths.py dense N M B OUT.json
    ONE H and A for the batch (QP 0's of qpb_generate's dense family), all four
    gradients, a seeded normal gx and glam:
    a   qpb_solve_backward_dual(shared = QPB_SHARED_H | QPB_SHARED_A)
    b   qpb_solve_factored_backward_dual, the buffer made beforehand
    c   qpb_factor_shared_backward + b: what a backward that starts from H and A pays
    Checked: b's outputs equal a's bit for bit.
  python tools/ab_dual_paths.py box N B OUT.json
    qpb_generate's box family, gH gf and the bounds' gradients, per-QP H:
    d   qpb_solve_backward_dual on the explicit A = [I; -I] (gA NULL)
    e   qpb_solve_box_backward_dual
    f   e without glam: qpb_solve_box_backward's kernels
    Checked: e against d (bwd_harness.rel's measure over the whole batch), and
    dx = -+glam exactly on the fixed variables.

Per leg: the median and minimum over all launches, the median of each round and
their spread (max - min).  Each difference is reported against three spreads of
the slower existing leg's round medians (a; d), whichever way it falls.
env: ROUNDS (5), REPS (6) -- 30 timed launches per leg"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "embedded-qp-solver_amd"))
import torch  # noqa: E402

import qpb  # noqa: E402

VP = ctypes.c_void_p


def rel(a, ref):
    """max over the batch of max|delta| / (1 + max|ref|) per QP."""
    a, ref = a.reshape(len(a), -1), ref.reshape(len(ref), -1)
    return float(((a - ref).abs().amax(1) / (1.0 + ref.abs().amax(1))).max())


def timed(legs, rounds, reps, s):
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
    out = {}
    for nm in legs:
        t = sorted(times[nm])
        out[nm] = {"median_ms": t[len(t) // 2], "min_ms": t[0], "round_medians_ms": rmed[nm],
                   "spread_ms": max(rmed[nm]) - min(rmed[nm])}
    return out


def against(L, x, a):
    diff = L[x]["median_ms"] - L[a]["median_ms"]
    bar = 3 * L[a]["spread_ms"]
    return {"ms": diff, "ratio": L[x]["median_ms"] / L[a]["median_ms"], "bar_ms_3_spreads_of_" + a: bar,
            "clears": bool(diff < -bar), "beyond_bar": bool(abs(diff) > bar)}


def dense(n, m, B, rounds, reps):
    dev = torch.device("cuda", 0)
    H, f, A, b = qpb.generate(n, B, 1, family="dense", m=m, shift=1.0, box=10.0, device=dev)
    H0, A0 = H[0].contiguous(), A[0].contiguous()
    del H, A
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    gx = torch.randn((B, n), dtype=torch.float64, device=dev, generator=gen)
    gl = torch.randn((B, m), dtype=torch.float64, device=dev, generator=gen)
    sol = qpb.solve_shared(H0, f, A0, b)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
    outs = {nm: (new(n, n), new(B, n), new(m, n), new(B, m)) for nm in "ab"}
    F = qpb.factor_shared_backward(H0, A0)
    F2 = qpb.factor_shared_backward(H0, A0)
    d = qpb.Desc(n, m, B, 0, 0, 0.0)
    s = torch.cuda.current_stream()
    p = lambda t: qpb._ptr(t)  # noqa: E731
    tail = lambda o: (p(gx), p(gl), *[p(t) for t in o], VP(s.cuda_stream))  # noqa: E731

    def a():
        rc = qpb.lib().qpb_solve_backward_dual(ctypes.byref(d), qpb.SHARED_H | qpb.SHARED_A, p(H0), p(A0), p(sol.x),
                                               p(sol.lam), p(sol.active), p(sol.status), *tail(outs["a"]))
        assert rc == 0, qpb.lib().qpb_last_error()

    def bq(fac=F):
        rc = qpb.lib().qpb_solve_factored_backward_dual(ctypes.byref(d), p(fac.fac), p(sol.x), p(sol.lam),
                                                        p(sol.active), p(sol.status), *tail(outs["b"]))
        assert rc == 0, qpb.lib().qpb_last_error()

    def c():
        rc = qpb.lib().qpb_factor_shared_backward(n, m, p(H0), p(A0), p(F2.fac), p(F2.status), VP(s.cuda_stream))
        assert rc == 0, qpb.lib().qpb_last_error()
        bq(F2)

    L = timed({"a": a, "b": bq, "c": c}, rounds, reps, s)
    a()
    bq()
    torch.cuda.synchronize()
    same = lambda u, v: bool(torch.equal(u.view(torch.int64), v.view(torch.int64)))  # noqa: E731
    mask = torch.from_numpy(qpb.active_mask_to_bool(sol.active[:4096].cpu().numpy(), m))
    return {"family": "dense", "n": n, "m": m, "B": B, "legs": L,
            "status_counts": torch.bincount(sol.status, minlength=5).tolist(),
            "mean_active_rows": float(mask.double().sum(1).mean()),
            "b_minus_a": against(L, "b", "a"), "c_minus_a": against(L, "c", "a"),
            "checks": {"b_bitwise_a": all(same(u, v) for u, v in zip(outs["b"], outs["a"])),
                       "b_finite": bool(all(torch.isfinite(t).all() for t in outs["b"]))}}


def box(n, B, rounds, reps):
    dev = torch.device("cuda", 0)
    m = 2 * n
    H, f, A, b = qpb.generate(n, B, 1, family="box", device=dev)
    ub, lb = b[:, :n].contiguous(), (-b[:, n:]).contiguous()
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    gx = torch.randn((B, n), dtype=torch.float64, device=dev, generator=gen)
    gl = torch.randn((B, m), dtype=torch.float64, device=dev, generator=gen)
    sol = qpb.solve_box(H, f, lb, ub)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
    gH, gf, gb = new(B, n, n), new(B, n), new(B, m)
    bH, bf, bl, bu = new(B, n, n), new(B, n), new(B, n), new(B, n)
    d = qpb.Desc(n, m, B, 0, 0, 0.0)
    s = torch.cuda.current_stream()
    p = lambda t: qpb._ptr(t)  # noqa: E731

    def general():
        rc = qpb.lib().qpb_solve_backward_dual(ctypes.byref(d), 0, p(H), p(A), p(sol.x), p(sol.lam), p(sol.active),
                                               p(sol.status), p(gx), p(gl), p(gH), p(gf), None, p(gb),
                                               VP(s.cuda_stream))
        assert rc == 0, qpb.lib().qpb_last_error()

    def boxd(glam=gl):
        rc = qpb.lib().qpb_solve_box_backward_dual(ctypes.byref(d), 0, p(H), p(sol.x), p(sol.active), p(sol.status),
                                                   p(gx), p(glam), p(bH), p(bf), p(bl), p(bu), VP(s.cuda_stream))
        assert rc == 0, qpb.lib().qpb_last_error()

    L = timed({"d": general, "e": boxd, "f": lambda: boxd(None)}, rounds, reps, s)
    general()
    boxd()
    torch.cuda.synchronize()
    mask = torch.from_numpy(qpb.active_mask_to_bool(sol.active.cpu().numpy(), m)).to(dev)
    ok = (sol.status == 0)[:, None]
    up, lo = mask[:, :n] & ok, mask[:, n:] & ~mask[:, :n] & ok
    exact = bool(torch.equal(bf[up], -gl[:, :n][up]) and torch.equal(bf[lo], gl[:, n:][lo]))
    return {"family": "box", "n": n, "m": m, "B": B, "legs": L,
            "status_counts": torch.bincount(sol.status, minlength=5).tolist(),
            "mean_fixed_variables": float((mask[:, :n] | mask[:, n:]).double().sum(1).mean()),
            "e_minus_d": against(L, "e", "d"), "e_minus_f": against(L, "e", "f"),
            "e_against_d": {"gH": rel(bH, gH), "gf": rel(bf, gf), "gub": rel(bu, gb[:, :n]),
                            "glb": rel(bl, -gb[:, n:])},
            "checks": {"dx_exact_on_fixed": exact, "e_finite": bool(all(torch.isfinite(t).all() for t in (bH, bf, bl, bu)))}}


def main(argv):
    rounds, reps = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("REPS", 6))
    if argv[0] == "dense":
        res = dense(int(argv[1]), int(argv[2]), int(argv[3]), rounds, reps)
    else:
        res = box(int(argv[1]), int(argv[2]), rounds, reps)
    res.update(rounds=rounds, reps=reps, library=qpb.version()[:8])
    out_path = argv[-1]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])
