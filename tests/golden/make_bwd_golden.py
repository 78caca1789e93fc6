#!/usr/bin/env python3
"""Generate tests/golden/bwd_cond_n{n}_m{m}.npz: the ill-conditioned family of
tests/bwd_cases.py (`conditioned`) with a 50-digit reference.

For every case the file holds the inputs (H, A, mask, x, lam, g, and the
family's parameters p = log10 cond(H) and size = |W|), dx and dlam from an
mpmath LU solve of the dense KKT system

    [ H    A_W^T ] [ dx   ]     [ g ]
    [ A_W   0    ] [ dlam ] = - [ 0 ]

at 50 digits, rounded to fp64 (dlam over all m rows, 0 outside W), the relative
residual of that solve evaluated at 50 digits, and `oracle_err`: the error of
tests/kkt_oracle.py's numpy solve against it, per gradient array (H, f, A, b)
as bwd_harness.rel.  The tests read the inputs from the file, never regenerate
them: the bits of a QR factorisation may differ between LAPACK builds.

Usage:  python tests/golden/make_bwd_golden.py     (about a minute; needs mpmath)
It adds its files' entries to manifest.json and leaves the others alone.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import bwd_cases as BC  # noqa: E402
from bwd_harness import NAMES, rel  # noqa: E402

DIGITS = 50
MAX_BYTES = 406728  # the largest fixture there was before these


def mp_solve(H, A, mask, g):
    """(dx, dlam (m,), residual): the KKT system of one QP at DIGITS digits."""
    import mpmath as mp
    mp.mp.dps = DIGITS
    n = H.shape[0]
    W = np.flatnonzero(mask)
    k = len(W)
    K = mp.zeros(n + k, n + k)
    for i in range(n):
        for j in range(n):
            K[i, j] = mp.mpf(float(H[i, j]))
    for t, r in enumerate(W):
        for j in range(n):
            K[n + t, j] = K[j, n + t] = mp.mpf(float(A[r, j]))
    rhs = mp.matrix([-mp.mpf(float(v)) for v in g] + [mp.mpf(0)] * k)
    sol = mp.lu_solve(K, rhs)
    res = mp.norm(K * sol - rhs, mp.inf) / (1 + mp.norm(rhs, mp.inf))
    dx = np.array([float(sol[i]) for i in range(n)])
    dlam = np.zeros(len(mask))
    dlam[W] = [float(sol[n + t]) for t in range(k)]
    return dx, dlam, float(res)


def build(n, m):
    H, A, mask, x, lam, g, p, size = BC.conditioned_inputs(n, m)
    c = BC.conditioned(n, m)  # the margins, and the numpy oracle as c.ref
    assert c.kept.sum() == mask.sum()
    sol = [mp_solve(H[i], A[i], mask[i], g[i]) for i in range(len(H))]
    dx, dlam, res = (np.array(v) for v in zip(*sol))
    assert res.max() <= 1e-40, res.max()
    ref = [BC.grads(x[i], lam[i], mask[i], dx[i], dlam[i]) for i in range(len(H))]
    err = np.stack([rel(c.ref[k], np.array([r[j] for r in ref])) for j, k in enumerate(NAMES)], axis=1)
    data = dict(H=H, A=A, mask=mask, x=x, lam=lam, g=g, p=p, size=size, dx=dx, dlam=dlam, residual=res,
                oracle_err=err)
    meta = dict(n=n, m=m, count=len(H), digits=DIGITS, residual_worst=float(res.max()),
                oracle_err_worst=float(err.max()), cond_exponents=list(BC.COND_EXPONENTS))
    return data, meta


def main():
    path = os.path.join(HERE, "manifest.json")
    with open(path) as fp:
        manifest = json.load(fp)
    for n, m in BC.COND_SHAPES:
        name = f"bwd_cond_n{n}_m{m}.npz"
        data, meta = build(n, m)
        out = os.path.join(HERE, name)
        np.savez_compressed(out, **data)
        assert os.path.getsize(out) <= MAX_BYTES, (name, os.path.getsize(out))
        with open(out, "rb") as fp:
            meta["sha256"] = hashlib.sha256(fp.read()).hexdigest()
        meta["arrays"] = {k: list(v.shape) for k, v in data.items()}
        meta["generator"] = "tests/golden/make_bwd_golden.py"
        manifest["files"][name] = meta
        print(name, meta["residual_worst"], meta["oracle_err_worst"], os.path.getsize(out))
    with open(path, "w") as fp:
        json.dump(manifest, fp, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
