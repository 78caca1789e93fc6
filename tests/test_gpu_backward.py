"""qpb_solve_backward on the GPU: the gradients of a solve through its KKT
system, in both kernels of qpb_kkt_bwd.hip (n <= 16, m <= 32: four QPs per
wavefront; the rest of n <= 32, m <= 64: one QP per wavefront).

The forward is qpb.solve_eq on the GPU (EO.eq_family(11, 67, ...): status OK
throughout, strict complementarity); the backward is fed the GPU's own x, lam
and active, and compared with tests/kkt_oracle.py (a dense numpy solve of the
same KKT system) on the same inputs.  Bars are the project's, those of
tests/test_gpu_eq.py: every gradient array within X_TOL = 1e-6 of the oracle,
max|delta| / (1 + max|ref|) per QP, and the certificate of the outputs (the two
relative residuals of the backward system) <= KKT_TOL = 1e-9.  For scale: two
fp64 algorithms on the CPU agree to 4e-13, with a certificate of 3e-14.

Every call here goes through the C-ABI (tests/bwd_harness.py, shared with
tests/test_gpu_backward_edges.py) into buffers of the test's own, filled
with 0xA5 and fenced by guard words: each test also checks that every element
was written and nothing outside.  "Bitwise" compares two launches on the same
QP.  The batch of 67 leaves the four-per-wave kernel a ragged last wave.
"""
import numpy as np
import pytest

import kkt_oracle as KO
from bwd_harness import KKT_TOL, NAMES, X_TOL
from bwd_harness import backward as _backward, dev as _dev, rel as _rel, same as _same

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

OK, MAX_ITER, NOT_SPD = 0, 1, 2
B = 67
SEED = 11

# (n, m, meq)
DENSE_SHAPES = [(1, 1, 0), (1, 2, 1), (3, 0, 0), (5, 9, 2), (16, 32, 0), (16, 32, 4), (16, 32, 16)]
WAVE_SHAPES = [(16, 33, 0), (17, 34, 3), (20, 40, 4), (32, 64, 8), (32, 64, 32)]
# one shape per load / store path: n < 16, n == 16, the wave kernel
PATH_SHAPES = [(5, 9, 2), (16, 32, 4), (20, 40, 4)]


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


def _forward(qpb, H, f, A, b, meq, **kw):
    """solve_eq (solve at m = 0) on the GPU; numpy (x, lam, active words, status)."""
    if A.shape[1] == 0:
        sol = qpb.solve(_dev(H), _dev(f), **kw)
    else:
        sol = qpb.solve_eq(_dev(H), _dev(f), _dev(A), _dev(b), meq, **kw)
    torch.cuda.synchronize()
    return sol.x.cpu().numpy(), sol.lam.cpu().numpy(), sol.active.cpu().numpy(), sol.status.cpu().numpy()


_CASES = {}


def _case(qpb, n, m, meq):
    """One shape's inputs, its forward on the GPU, the cotangent and the
    oracle's gradients: computed once, shared, never modified."""
    key = (n, m, meq)
    if key not in _CASES:
        H, f, A, b, xc = KO.family(SEED, B, n, m, meq)
        x, lam, act, st = _forward(qpb, H, f, A, b, meq)
        assert (st == OK).all(), st
        mask = qpb.active_mask_to_bool(act, m) if m else np.zeros((B, 0), bool)
        g = np.random.default_rng([SEED, n, m, meq]).standard_normal((B, n))
        ref = [KO.backward(H[i], x[i], lam[i], A[i], mask[i], g[i]) for i in range(B)]
        ref = {k: np.array([r[j] for r in ref]) for j, k in enumerate(NAMES)}
        _CASES[key] = dict(H=H, f=f, A=A, b=b, x=x, lam=lam, act=act, st=st, mask=mask, g=g, ref=ref)
    return _CASES[key]


def _run(qpb, c, **kw):
    return _backward(qpb, c["H"], c["A"], c["x"], c["lam"], c["act"], kw.pop("st", c["st"]), c["g"], **kw)


# ------------------------------------------------------- 1. parity and certificate (7. symmetry)
@pytest.mark.parametrize("n,m,meq", DENSE_SHAPES + WAVE_SHAPES)
def test_parity_and_certificate(qpb, n, m, meq):
    c = _case(qpb, n, m, meq)
    out = _run(qpb, c)
    names = NAMES if m else NAMES[:2]
    assert set(out) == set(names)
    errs = {k: float(_rel(out[k], c["ref"][k]).max()) for k in names}
    gb = out["b"] if m else np.zeros((B, 0))
    cert = np.array([KO.certificate(c["H"][i], c["A"][i], c["mask"][i], c["g"][i], out["f"][i], gb[i])
                     for i in range(B)])
    print(f"({n},{m},{meq}): active rows {c['mask'].sum(axis=1).min()}..{c['mask'].sum(axis=1).max()} "
          f"errors {errs} certificate stat {cert[:, 0].max():.2e} prim {cert[:, 1].max():.2e} "
          f"lam_eq<0 {(c['lam'][:, :meq] < 0).mean() if meq else 0:.2f}")
    for k in names:
        assert np.isfinite(out[k]).all(), k
        assert errs[k] <= X_TOL, (k, errs[k])
    assert cert.max() <= KKT_TOL, cert.max(axis=0)
    assert np.array_equal(out["H"], out["H"].transpose(0, 2, 1))
    if m:
        # rows outside W are exactly zero, and the equalities are all in W with multipliers of either sign
        assert (out["A"][~c["mask"]] == 0.0).all() and (out["b"][~c["mask"]] == 0.0).all()
        assert c["mask"][:, :meq].all()
        if 0 < meq < n:
            assert (c["lam"][:, :meq] < 0).any() and (c["lam"][:, :meq] > 0).any()
    # the Python call returns the same bits
    sol = qpb.Solution(_dev(c["x"]), _dev(c["lam"]), _dev(c["act"]), _dev(c["st"]), None)
    got = qpb.solve_backward(_dev(c["H"]), _dev(c["A"]) if m else None, sol, _dev(c["g"]))
    torch.cuda.synchronize()
    assert [t is None for t in got] == [k not in names for k in NAMES]
    assert _same(out, {k: t.cpu().numpy() for k, t in zip(NAMES, got) if t is not None})


# ------------------------------------------------------- 2. everything written, zeros where due
@pytest.mark.parametrize("n,m,meq", PATH_SHAPES)
@pytest.mark.parametrize("how", ["not_spd", "max_iter"])
def test_non_ok_qps_get_zeros(qpb, n, m, meq, how):
    c = _case(qpb, n, m, meq)
    H = c["H"].copy()
    kw = {}
    if how == "not_spd":
        H[3] = -np.eye(n)
    else:
        kw["max_iter"] = 1
    x, lam, act, st = _forward(qpb, H, c["f"], c["A"], c["b"], meq, **kw)
    assert ((st == NOT_SPD) == (np.arange(B) == 3)).all() if how == "not_spd" else (st == MAX_ITER).any(), st
    out = _backward(qpb, H, c["A"], x, lam, act, st, c["g"])  # (guards and written-ness checked inside)
    bad = st != OK
    mask = qpb.active_mask_to_bool(act, m)
    for k in NAMES:
        assert (out[k][bad] == 0.0).all(), k
        assert np.isfinite(out[k]).all(), k
    good = ~bad
    assert (out["A"][good][~mask[good]] == 0.0).all() and (out["b"][good][~mask[good]] == 0.0).all()
    if how == "not_spd":  # the others are the unchanged QPs of the shared case
        ref = {k: v[good] for k, v in _run(qpb, c).items()}
        assert _same({k: v[good] for k, v in out.items()}, ref)


# ------------------------------------------------------- 3. NULL outputs, NULL status
@pytest.mark.parametrize("n,m,meq", PATH_SHAPES)
def test_null_outputs_and_null_status(qpb, n, m, meq):
    c = _case(qpb, n, m, meq)
    full = _run(qpb, c)
    for k in NAMES:
        one = _run(qpb, c, need=(k,))
        assert _same(one, {k: full[k]}), k
        three = tuple(j for j in NAMES if j != k)
        assert _same(_run(qpb, c, need=three), {j: full[j] for j in three}), three
    assert _same(_run(qpb, c, st=None), full)
    # the Python call: what is left out of `need` comes back as None
    sol = qpb.Solution(_dev(c["x"]), _dev(c["lam"]), _dev(c["act"]), None, None)
    gH, gf, gA, gb = qpb.solve_backward(_dev(c["H"]), _dev(c["A"]), sol, _dev(c["g"]), need=("f", "b"))
    torch.cuda.synchronize()
    assert gH is None and gA is None
    assert _same({"f": gf.cpu().numpy(), "b": gb.cpu().numpy()}, {"f": full["f"], "b": full["b"]})


# ------------------------------------------------------- 4. independence
@pytest.mark.parametrize("n,m,meq", PATH_SHAPES)
def test_a_qp_depends_on_its_own_inputs_only(qpb, n, m, meq):
    c = _case(qpb, n, m, meq)
    full = _run(qpb, c)
    k = 5
    one = slice(k, k + 1)
    alone = _backward(qpb, c["H"][one], c["A"][one], c["x"][one], c["lam"][one], c["act"][one], c["st"][one],
                      c["g"][one])
    assert _same(alone, {j: v[one] for j, v in full.items()})
    arrays = {j: c[j].copy() for j in ("H", "A", "x", "lam", "g")}
    others = np.arange(B) != k
    for v in arrays.values():
        v[others] = np.nan
    poisoned = _backward(qpb, arrays["H"], arrays["A"], arrays["x"], arrays["lam"], c["act"], c["st"], arrays["g"])
    assert _same({j: v[one] for j, v in poisoned.items()}, alone)


# ------------------------------------------------------- 5. streams
@pytest.mark.parametrize("n,m,meq", PATH_SHAPES)
def test_non_default_stream_gives_the_same_bits(qpb, n, m, meq):
    c = _case(qpb, n, m, meq)
    full = _run(qpb, c)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert _same(_run(qpb, c, stream=s), full)


# ------------------------------------------------------- 6. the size limit
def test_above_the_wave_class_is_unsupported(qpb):
    n, Bq = 33, 2
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    sol = qpb.Solution(z(Bq, n), None, None, None, None)
    with pytest.raises(qpb.QPBError) as e:
        qpb.solve_backward(z(Bq, n, n), None, sol, z(Bq, n))
    assert e.value.code == qpb.ERR_UNSUPPORTED and "n<=32" in str(e.value)


# ------------------------------------------------------- 8. a dependent row in a hand-made mask
@pytest.mark.parametrize("n,m,meq", PATH_SHAPES)
@pytest.mark.parametrize("later", [True, False])
def test_duplicated_active_row_is_skipped(qpb, n, m, meq, later):
    """Row j2 is made a copy of the active row j1 and marked active as well,
    with a multiplier of the test's own.  In row order the second of the two is
    the dependent one: dlam = 0, so gb = 0 and gA = lam dx^T for it, and
    everything else is the system without that row."""
    c = _case(qpb, n, m, meq)
    Bq = 8
    A, lam, mask = c["A"][:Bq].copy(), c["lam"][:Bq].copy(), c["mask"][:Bq].copy()
    skipped = np.zeros(Bq, int)
    for i in range(Bq):
        on, off = np.flatnonzero(mask[i]), np.flatnonzero(~mask[i])
        j1 = on[len(on) // 2]
        cand = off[off > j1] if later else off[off < j1]
        if len(cand) == 0:  # no inactive row on that side: the other one
            cand = off
        j2 = cand[0]
        A[i, j2] = A[i, j1]
        lam[i, j2] = 0.37
        mask[i, j2] = True
        skipped[i] = max(j1, j2)
    act = np.zeros((Bq, (m + 31) // 32), np.uint32)
    for i, j in zip(*np.nonzero(mask)):
        act[i, j // 32] |= np.uint32(1) << np.uint32(j % 32)
    act = act.view(np.int32)
    out = _backward(qpb, c["H"][:Bq], A, c["x"][:Bq], lam, act, c["st"][:Bq], c["g"][:Bq])
    for i in range(Bq):
        keep = mask[i].copy()
        keep[skipped[i]] = False
        gH, gf, gA, gb = KO.backward(c["H"][i], c["x"][i], lam[i], A[i], keep, c["g"][i])
        gA[skipped[i]] = lam[i, skipped[i]] * gf
        for k, ref in zip(NAMES, (gH, gf, gA, gb)):
            assert np.isfinite(out[k][i]).all(), (i, k)
            assert _rel(out[k][i][None], ref[None])[0] <= X_TOL, (i, k)
        assert out["b"][i, skipped[i]] == 0.0
        assert (out["A"][i][~mask[i]] == 0.0).all() and (out["b"][i][~mask[i]] == 0.0).all()
