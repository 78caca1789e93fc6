"""tests/bwd_cases.py on the CPU: the inputs of tests/test_gpu_backward_edges.py
are what they claim to be, their references agree with one another, and the
record of why kkt_bwd projects u = L^{-1} g twice.

  * the committed 50-digit fixtures have the manifest's hashes and, where
    mpmath imports, two regenerated solves equal the stored ones;
  * every builder keeps its rows far from the kernels' dependency threshold
    (kept >= 1e-9, in `conditioned` >= 1e-12; skipped <= 1e-28 against 1e-24);
  * one_hot's closed form and scaled's scaling law agree with
    tests/kkt_oracle.py, which they do not use;
  * on the ill-conditioned family, the kernels' algebra in numpy
    (bwd_cases.emulate) with TWO projections of u meets both bars of the GPU
    test on every case -- so the inputs are passable -- and with ONE misses the
    certificate (A_W dx = 0) on every cond(H) = 1e10 case with |W| >= n - 1.
"""
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest

import bwd_cases as BC
import kkt_oracle as KO
from bwd_harness import KKT_TOL, NAMES, rel

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WITH_ROWS = [(n, m) for n, m in BC.ALL_ROUTES if m > 0]
WITH_PAIRS = [(n, m) for n, m in BC.ALL_ROUTES if m > 16]


def _stack(rows):
    return {k: np.array([r[j] for r in rows]) for j, k in enumerate(NAMES)}


def _oracle(c):
    """kkt_oracle.backward on a case's rows that count (the case's own mask where all do)."""
    assert np.array_equal(c.kept, c.mask)
    return _stack([KO.backward(c.H[i], c.x[i], c.lam[i], c.A[i], c.mask[i], c.g[i]) for i in range(len(c.H))])


# ------------------------------------------------------------------ the fixture
@pytest.mark.parametrize("n,m", BC.COND_SHAPES)
def test_fixture_matches_its_manifest_entry(n, m):
    name = f"bwd_cond_n{n}_m{m}.npz"
    meta = json.load(open(os.path.join(GOLDEN, "manifest.json")))["files"][name]
    with open(os.path.join(GOLDEN, name), "rb") as fp:
        assert hashlib.sha256(fp.read()).hexdigest() == meta["sha256"]
    z = np.load(os.path.join(GOLDEN, name))
    assert {k: list(z[k].shape) for k in z.files} == meta["arrays"]
    assert meta["digits"] >= 40 and z["residual"].max() <= 1e-40
    c, p, size, oerr = BC.conditioned_fixture(n, m)
    assert sorted(zip(p, size)) == sorted((q, s) for q in BC.COND_EXPONENTS for s in BC.sizes_of(n, m))
    assert np.array_equal(c.mask.sum(axis=1), size)
    assert np.array_equal(c.H, c.H.transpose(0, 2, 1))
    cond = np.array([np.linalg.cond(H) for H in c.H])
    assert np.allclose(np.log10(cond), p, atol=1e-3), cond
    assert (c.ref["b"][~c.mask] == 0.0).all() and np.isfinite(oerr).all()
    # every row of every mask counts, 12 orders above the kernels' threshold at the least
    lo, hi = BC.margins(c)
    print(f"({n},{m}): smallest kept ratio {lo:.1e}")
    assert lo >= BC.COND_KEPT_MIN and hi == 0.0


def test_regenerated_references_equal_the_stored_ones():
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_bwd_golden", os.path.join(GOLDEN, "make_bwd_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for (n, m), want in (((13, 26), (10, 13)), ((16, 32), (10, 15))):
        z = np.load(os.path.join(GOLDEN, f"bwd_cond_n{n}_m{m}.npz"))
        i = int(np.flatnonzero((z["p"] == want[0]) & (z["size"] == want[1]))[0])
        dx, dlam, res = gen.mp_solve(z["H"][i], z["A"][i], z["mask"][i], z["g"][i])
        assert np.array_equal(dx, z["dx"][i]) and np.array_equal(dlam, z["dlam"][i]) and res <= 1e-40


# ------------------------------------------------------------------ the builders
def test_routes_reach_every_form():
    """The launcher's choice (qpb_kkt_bwd.hip) restated: every form has a shape."""
    def form(n, m):
        if n > 16 or m > 32:
            return "wave-2words" if m > 32 and n > 16 else ("wave-n<=16-2words" if m > 32 else "wave-1word")
        return f"dense<{1 if m <= 16 else 2},{'true' if n == 16 else 'false'}>"
    for name, shp in BC.ROUTES.items():
        assert shp and all(form(n, m) == name for n, m in shp), name
    assert set(BC.ALL_ROUTES) >= set(BC.FORM_ROUTES) and {form(n, m) for n, m in BC.FORM_ROUTES} == set(BC.ROUTES)


@pytest.mark.parametrize("n,m", BC.ALL_ROUTES)
def test_sizes_margins(n, m):
    c = BC.sizes(n, m)
    assert list(c.mask.sum(axis=1)) == BC.sizes_of(n, m) * 2
    assert np.array_equal(c.kept, c.mask)
    assert (c.lam[c.mask] > 0).all() and (c.lam[~c.mask] == 7.0).all()
    lo, hi = BC.margins(c)
    assert lo >= BC.KEPT_MIN and hi == 0.0, (lo, hi)


@pytest.mark.parametrize("n,m", WITH_PAIRS)
def test_pairs_margins(n, m):
    c = BC.pairs(n, m)
    sets = [tuple(np.flatnonzero(r)) for r in c.mask]
    assert sets == [(k, k + 16) for k in range(m - 16)] + ([(31, 32)] if m > 32 else [])
    lo, hi = BC.margins(c)
    assert lo >= BC.KEPT_MIN and hi == 0.0 and np.array_equal(c.kept, c.mask)


@pytest.mark.parametrize("n,m", BC.FORM_ROUTES)
def test_overfull_and_weak_margins(n, m):
    c = BC.overfull(n, m)
    assert c.mask.all() and not c.kept[:, 5].any() and (c.lam > 0).all()
    assert np.array_equal(c.A[:, 5], c.A[:, 1] + 2.0 * c.A[:, 3])
    assert (c.kept.sum(axis=1) == min(n, m - 1)).all()
    lo, hi = BC.margins(c)
    print(f"overfull ({n},{m}): kept >= {lo:.1e}, skipped <= {hi:.1e}")
    assert lo >= BC.KEPT_MIN and 0.0 < hi <= BC.SKIPPED_MAX
    w = BC.weak(n, m)
    assert np.array_equal(w.kept, w.mask)
    assert ((w.mask & (w.lam == 0.0)).sum(axis=1) > 0).all() and ((w.mask & (w.lam > 0.0)).sum(axis=1) > 0).all()
    lo, hi = BC.margins(w)
    assert lo >= BC.KEPT_MIN and hi == 0.0


# ------------------------------------------------------------------ the references against one another
@pytest.mark.parametrize("n,m", WITH_ROWS)
def test_one_hot_closed_form_against_the_oracle(n, m):
    """H = I + B^T B / n has cond(H) < 10 and the rows unit norm: two fp64
    solves of this system agree to a few hundred eps; the bar is 1e-12."""
    c = BC.one_hot(n, m)
    assert np.array_equal(c.mask, np.eye(m, dtype=bool))
    ref = _oracle(c)
    errs = {k: float(rel(ref[k], c.ref[k]).max()) for k in NAMES}
    print(f"one_hot ({n},{m}): {errs}")
    assert max(errs.values()) <= 1e-12, errs


@pytest.mark.parametrize("n,m", [(7, 14), (16, 32), (20, 33)])
def test_scaling_law_against_the_oracle(n, m):
    """The mildest scaling (H x 16, rows x 4 or / 4, g / 8).  Both sides are
    numpy solves of a dense KKT matrix, the law's of K and the oracle's of the
    scaled K', each good to eps cond at best: the bar per QP is
    eps (cond K + cond K'), and nothing looser than 1e-4 counts as agreement."""
    base = BC.sizes(n, m)
    c = BC.scaled(base, *BC.SCALINGS[0])
    ref = _oracle(c)

    def cond(q, i):
        W = np.flatnonzero(q.mask[i])
        K = np.zeros((n + len(W), n + len(W)))
        K[:n, :n], K[:n, n:], K[n:, :n] = q.H[i], q.A[i][W].T, q.A[i][W]
        return np.linalg.cond(K)
    bar = np.finfo(float).eps * np.array([cond(base, i) + cond(c, i) for i in range(len(c.H))])
    errs = {k: BC.pure(ref[k], c, k) for k in NAMES}
    print(f"scaled ({n},{m}) {BC.SCALINGS[0]}: worst {max(e.max() for e in errs.values()):.1e}, bars up to {bar.max():.1e}")
    assert bar.max() <= 1e-4
    for k in NAMES:
        assert (errs[k] <= bar).all(), (k, errs[k] / bar)
    assert np.array_equal(c.ref["H"], c.ref["H"].transpose(0, 2, 1))


# ------------------------------------------------------------------ why u is projected twice
def _emulated(c, passes):
    out, cert = [], []
    for i in range(len(c.H)):
        dx, dl = BC.emulate(c.H[i], c.A[i], c.mask[i], c.g[i], passes)
        out.append(BC.grads(c.x[i], c.lam[i], c.mask[i], dx, dl))
        cert.append(KO.certificate(c.H[i], c.A[i], c.mask[i], c.g[i], dx, -dl))
    return _stack(out), np.array(cert)


@pytest.mark.parametrize("n,m", BC.COND_SHAPES)
def test_two_projections_meet_the_bars_and_one_does_not(n, m):
    c, p, size, oerr = BC.conditioned_fixture(n, m)
    two, cert2 = _emulated(c, 2)
    one, cert1 = _emulated(c, 1)
    hard = (p == 10) & (size >= n - 1)
    for i in range(len(c.H)):
        print(f"({n},{m}) cond 1e{p[i]} |W| {size[i]}: prim one pass {cert1[i, 1]:.1e} two {cert2[i, 1]:.1e}, "
              f"stat {cert1[i, 0]:.1e} / {cert2[i, 0]:.1e}")
    # (a) the certificate, (b) the error against the 50-digit reference
    assert cert2.max() <= KKT_TOL, cert2.max(axis=0)
    for j, k in enumerate(NAMES):
        err = rel(two[k], c.ref[k])
        bar = np.maximum(BC.COND_FLOOR, 10.0 * oerr[:, j])
        assert (err <= bar).all(), (k, err / bar)
    assert hard.sum() == 2 and (cert1[hard, 1] > KKT_TOL).all(), cert1[hard]
    assert cert1[:, 0].max() <= KKT_TOL  # stationarity never needed the second pass
