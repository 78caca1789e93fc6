#!/usr/bin/env python3
"""What T right-hand sides per QP in one launch cost against the workaround they
replace, on data generated on the device, rounds interleaved as in
tools/ab_dual_paths.py (clock and thermal drift hit every leg alike).

  python tools/ab_backward_multi.py factored N M BT T OUT.json
    ONE H and A for the batch (QP 0's of qpb_generate's dense family), factored
    beforehand; B = BT / T solved QPs, a seeded normal gx and glam per direction:
    a   the workaround: qpb_solve_factored_backward_dual (gH = gA = NULL) on B T
        QPs, with x, lam, active and status replicated T times
    b   qpb_solve_factored_backward_multi on B QPs with T directions
    c   b with QPB_SHARED_RHS (QP 0's T directions for every QP)
  python tools/ab_backward_multi.py box N BT T per|one OUT.json
    qpb_generate's box family, per-QP H or one H (QP 0's):
    a   qpb_solve_box_backward_dual (gH = NULL) on B T QPs, with x, active, status
        and (per) H replicated T times
    b   qpb_solve_box_backward_multi on B QPs with T directions
    c   b with QPB_SHARED_RHS
    Checked in both: b's outputs equal a's bit for bit, c's equal b's on copies.
  python tools/ab_backward_multi.py sweep OUT_DIR RUN
    Every row of the README's table (SWEEP x T in {1, 4, 16}) in one process,
    one OUT_DIR/ab_multi_<row>_BT<B T>_T<T>_run<RUN>.json each.

Per leg: the median and minimum over all launches, the median of each round and
their spread (max - min), and the bytes of the arrays the leg reads and writes.
a - b is reported against three spreads of leg a's round medians, whichever way
it falls: "clears" only when b is faster by more than that.
env: ROUNDS (5), REPS (6) -- 30 timed launches per leg"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "embedded-qp-solver_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import qpb  # noqa: E402
from ab_dual_paths import timed  # noqa: E402

VP = ctypes.c_void_p


def nbytes(*ts):
    return int(sum(t.numel() * t.element_size() for t in ts if t is not None))


def verdict(L):
    diff = L["a"]["median_ms"] - L["b"]["median_ms"]
    bar = 3 * L["a"]["spread_ms"]
    return {"a_minus_b_ms": diff, "b_over_a": L["b"]["median_ms"] / L["a"]["median_ms"],
            "c_over_a": L["c"]["median_ms"] / L["a"]["median_ms"], "bar_ms_3_spreads_of_a": bar,
            "verdict": "clears" if diff > bar else ("b slower beyond the bar" if diff < -bar else "within")}


def same(u, v):
    return bool(torch.equal(u.reshape(-1).view(torch.int64), v.reshape(-1).view(torch.int64)))


def rep(t, T):
    """Each QP's entry T times in a row: QP k's copies are QPs k T .. k T + T - 1."""
    return None if t is None else t.repeat_interleave(T, dim=0).contiguous()


def factored(n, m, BT, T, rounds, reps):
    dev = torch.device("cuda", 0)
    B = BT // T
    H, f, A, b = qpb.generate(n, B, 1, family="dense", m=m, shift=1.0, box=10.0, device=dev)
    H0, A0 = H[0].contiguous(), A[0].contiguous()
    del H, A
    sol = qpb.solve_shared(H0, f, A0, b)
    F = qpb.factor_shared_backward(H0, A0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    gx = torch.randn((B, T, n), dtype=torch.float64, device=dev, generator=gen)
    gl = torch.randn((B, T, m), dtype=torch.float64, device=dev, generator=gen)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
    xa, la, aa, sa = rep(sol.x, T), rep(sol.lam, T), rep(sol.active, T), rep(sol.status, T)
    oa, ob, oc = (new(B * T, n), new(B * T, m)), (new(B, T, n), new(B, T, m)), (new(B, T, n), new(B, T, m))
    gx0, gl0 = gx[0].contiguous(), gl[0].contiguous()
    da, db = qpb.Desc(n, m, B * T, 0, 0, 0.0), qpb.Desc(n, m, B, 0, 0, 0.0)
    s = torch.cuda.current_stream()
    p = lambda t: qpb._ptr(t)  # noqa: E731

    def a():
        rc = qpb.lib().qpb_solve_factored_backward_dual(ctypes.byref(da), p(F.fac), p(xa), p(la), p(aa), p(sa), p(gx),
                                                        p(gl), None, p(oa[0]), None, p(oa[1]), VP(s.cuda_stream))
        assert rc == 0, qpb.lib().qpb_last_error()

    def multi(shared, g, l, o):
        rc = qpb.lib().qpb_solve_factored_backward_multi(ctypes.byref(db), p(F.fac), p(sol.active), p(sol.status), T,
                                                         shared, p(g), p(l), p(o[0]), p(o[1]), VP(s.cuda_stream))
        assert rc == 0, qpb.lib().qpb_last_error()

    legs = {"a": a, "b": lambda: multi(0, gx, gl, ob), "c": lambda: multi(qpb.SHARED_RHS, gx0, gl0, oc)}
    L = timed(legs, rounds, reps, s)
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    checks = {"b_bitwise_a": same(ob[0], oa[0]) and same(ob[1], oa[1]),
              "b_finite": bool(torch.isfinite(ob[0]).all() and torch.isfinite(ob[1]).all())}
    multi(0, gx0.expand(B, T, n).contiguous(), gl0.expand(B, T, m).contiguous(), ob)
    torch.cuda.synchronize()
    checks["c_bitwise_b_on_copies"] = same(oc[0], ob[0]) and same(oc[1], ob[1])
    L["a"]["bytes"] = nbytes(F.fac, xa, la, aa, sa, gx, gl, *oa)
    L["b"]["bytes"] = nbytes(F.fac, sol.active, sol.status, gx, gl, *ob)
    L["c"]["bytes"] = nbytes(F.fac, sol.active, sol.status, gx0, gl0, *oc)
    return {"path": "factored", "n": n, "m": m, "B": B, "T": T, "BT": B * T, "legs": L, **verdict(L),
            "status_counts": torch.bincount(sol.status, minlength=5).tolist(), "checks": checks}


def box(n, BT, T, one, rounds, reps):
    dev = torch.device("cuda", 0)
    m = 2 * n
    B = BT // T
    H, f, A, b = qpb.generate(n, B, 1, family="box", device=dev)
    del A
    ub, lb = b[:, :n].contiguous(), (-b[:, n:]).contiguous()
    if one:
        H = H[0].contiguous()
    sol = qpb.solve_box_shared(H, f, lb, ub) if one else qpb.solve_box(H, f, lb, ub)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    gx = torch.randn((B, T, n), dtype=torch.float64, device=dev, generator=gen)
    gl = torch.randn((B, T, m), dtype=torch.float64, device=dev, generator=gen)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
    Ha = H if one else rep(H, T)
    xa, aa, sa = rep(sol.x, T), rep(sol.active, T), rep(sol.status, T)
    oa = tuple(new(B * T, n) for _ in range(3))
    ob, oc = tuple(new(B, T, n) for _ in range(3)), tuple(new(B, T, n) for _ in range(3))
    gx0, gl0 = gx[0].contiguous(), gl[0].contiguous()
    da, db = qpb.Desc(n, m, B * T, 0, 0, 0.0), qpb.Desc(n, m, B, 0, 0, 0.0)
    sh = qpb.SHARED_H if one else 0
    s = torch.cuda.current_stream()
    p = lambda t: qpb._ptr(t)  # noqa: E731

    def a():
        rc = qpb.lib().qpb_solve_box_backward_dual(ctypes.byref(da), sh, p(Ha), p(xa), p(aa), p(sa), p(gx), p(gl), None,
                                                   *[p(t) for t in oa], VP(s.cuda_stream))
        assert rc == 0, qpb.lib().qpb_last_error()

    def multi(shared, g, l, o):
        rc = qpb.lib().qpb_solve_box_backward_multi(ctypes.byref(db), sh | shared, p(H), p(sol.active), p(sol.status), T,
                                                    p(g), p(l), *[p(t) for t in o], VP(s.cuda_stream))
        assert rc == 0, qpb.lib().qpb_last_error()

    legs = {"a": a, "b": lambda: multi(0, gx, gl, ob), "c": lambda: multi(qpb.SHARED_RHS, gx0, gl0, oc)}
    L = timed(legs, rounds, reps, s)
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    checks = {"b_bitwise_a": all(same(u, v) for u, v in zip(ob, oa)),
              "b_finite": bool(all(torch.isfinite(t).all() for t in ob))}
    multi(0, gx0.expand(B, T, n).contiguous(), gl0.expand(B, T, m).contiguous(), ob)
    torch.cuda.synchronize()
    checks["c_bitwise_b_on_copies"] = all(same(u, v) for u, v in zip(oc, ob))
    L["a"]["bytes"] = nbytes(Ha, xa, aa, sa, gx, gl, *oa)
    L["b"]["bytes"] = nbytes(H, sol.active, sol.status, gx, gl, *ob)
    L["c"]["bytes"] = nbytes(H, sol.active, sol.status, gx0, gl0, *oc)
    return {"path": "box", "H": "one" if one else "per QP", "n": n, "m": m, "B": B, "T": T, "BT": B * T, "legs": L,
            **verdict(L), "status_counts": torch.bincount(sol.status, minlength=5).tolist(), "checks": checks}


# the README's table: B T at the project's large batches, T in {1, 4, 16} at every shape
SWEEP = ([("factored", 16, 32, 1 << 20), ("factored", 32, 64, 1 << 18), ("factored", 20, 40, 1 << 18),
          ("box", 16, "per", 1 << 20)]
         + [("box", n, h, 1 << 18) for n in (32, 20) for h in ("per", "one")])
SWEEP_T = (1, 4, 16)


def sweep(out_dir, run, rounds, reps):
    """Every row of the table in one process: OUT_DIR/ab_multi_<path>_..._run<RUN>.json each."""
    os.makedirs(out_dir, exist_ok=True)
    for path, n, second, BT in SWEEP:
        for T in SWEEP_T:
            if path == "factored":
                res, tag = factored(n, second, BT, T, rounds, reps), f"factored_n{n}_m{second}"
            else:
                res, tag = box(n, BT, T, second == "one", rounds, reps), f"box_n{n}_{second}"
            res.update(rounds=rounds, reps=reps, library=qpb.version()[:8], run=run)
            with open(os.path.join(out_dir, f"ab_multi_{tag}_BT{BT}_T{T}_run{run}.json"), "w") as fh:
                json.dump(res, fh, indent=1)
            print(tag, "BT", BT, "T", T, {k: round(v["median_ms"], 4) for k, v in res["legs"].items()},
                  "spread a", round(res["legs"]["a"]["spread_ms"], 4), res["verdict"], res["checks"], flush=True)
            torch.cuda.empty_cache()


def main(argv):
    rounds, reps = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("REPS", 6))
    if argv[0] == "sweep":  # sweep OUT_DIR RUN
        return sweep(argv[1], argv[2], rounds, reps)
    if argv[0] == "factored":
        res = factored(int(argv[1]), int(argv[2]), int(argv[3]), int(argv[4]), rounds, reps)
    else:
        res = box(int(argv[1]), int(argv[2]), int(argv[3]), argv[4] == "one", rounds, reps)
    res.update(rounds=rounds, reps=reps, library=qpb.version()[:8])
    out_path = argv[-1]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])
