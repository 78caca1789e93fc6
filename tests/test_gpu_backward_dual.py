"""qpb_solve_backward_dual on the GPU: the backward of a solve for a loss that
reads the multipliers too, in the DU forms of both kernels of qpb_kkt_bwd.hip
(n <= 16, m <= 32: four QPs per wavefront, MR = 1 and 2, n == 16 and padded;
the rest of n <= 32, m <= 64: one QP per wavefront), plain and with a shared
H and / or A.

The forward is qpb.solve_eq on the GPU (KO.family(11, 67, ...): status OK
throughout, strict complementarity); the backward is fed the GPU's own x, lam
and active and seeded normal cotangents gx and glam, and compared with
tests/dual_oracle.py (a dense numpy solve of the same KKT system).  Bars are
the project's (tests/bwd_harness.py): every gradient array within X_TOL = 1e-6
of the oracle, max|delta| / (1 + max|ref|) per QP, and the certificate of the
outputs (the two relative residuals of the system, the second with glam_W)
<= KKT_TOL = 1e-9.  A summed gradient of a shared operand is held to
tests/shared_cases.py's derived bound (B + 4) 2^-53 sum|products|.

Every call goes through the C-ABI into buffers of the test's own, filled with
0xA5 and fenced by guard words: each test also checks that every element was
written and nothing outside.  "Bitwise" compares two launches on the same QP.
The batch of 67 leaves the four-per-wave kernel a ragged last wave.
"""
import ctypes
import itertools
import math

import numpy as np
import pytest

import dual_oracle as DO
import kkt_oracle as KO
import shared_cases as SC
from bwd_harness import FILL8, GUARD, KKT_TOL, NAMES, X_TOL
from bwd_harness import backward as _plain_backward, dev as _dev, rel as _rel, same as _same

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

OK, MAX_ITER, NOT_SPD, NUMERICAL = 0, 1, 2, 4
B = 67
SEED = 11

# (n, m, meq): the smallest shapes that reach each path
DENSE_SHAPES = [(1, 2, 1), (5, 9, 2), (16, 16, 3), (16, 32, 4), (16, 32, 16)]  # MR 1 padded, MR 1 / 2 at n = 16, meq = n
WAVE_SHAPES = [(16, 33, 0), (20, 40, 4), (32, 64, 8), (32, 64, 32)]
# one shape per load / store path: n < 16, n == 16, the wave kernel
PATH_SHAPES = [(5, 9, 2), (16, 32, 4), (20, 40, 4)]


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


def _dual(qpb, shared, H, A, x, lam, act, st, g, gl, need=NAMES, stream=None):
    """qpb_solve_backward_dual through the C-ABI on numpy inputs: H is (n, n)
    with SHARED_H in `shared`, else (B, n, n), and A likewise; st None: status
    NULL; gl None: glam NULL.  Outputs live between guard words in buffers filled
    with 0xA5.  Returns a dict of the numpy outputs in `need`."""
    Bq, n = g.shape
    m = A.shape[-2]
    ins = [_dev(H), _dev(A) if m else None, _dev(x), _dev(lam) if m else None, _dev(act) if m else None,
           _dev(st) if st is not None else None, _dev(g), _dev(gl) if gl is not None and m else None]
    shp = {"H": H.shape, "f": (Bq, n), "A": A.shape, "b": (Bq, m)}
    bufs, views = {}, {}
    for k, shape in shp.items():
        if k in need and math.prod(shape) > 0:
            t = torch.empty(math.prod(shape) + 2 * GUARD, dtype=torch.float64, device="cuda")
            t.view(torch.uint8).fill_(0xA5)
            bufs[k], views[k] = t, t[GUARD:GUARD + math.prod(shape)].view(shape)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    d = qpb.Desc(n, m, Bq, 0, 0, 0.0)
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = qpb.lib().qpb_solve_backward_dual(ctypes.byref(d), shared, *[ptr(t) for t in ins],
                                           *[ptr(views.get(k)) for k in NAMES], ctypes.c_void_p(s.cuda_stream))
    assert rc == 0, qpb.lib().qpb_last_error()
    s.synchronize()
    out = {}
    for k, t in bufs.items():
        raw = t.cpu().numpy().view(np.int64)
        assert (raw[:GUARD] == FILL8).all() and (raw[-GUARD:] == FILL8).all(), (k, "guard words written")
        assert not (raw[GUARD:-GUARD] == FILL8).any(), (k, "elements never written")
        out[k] = views[k].cpu().numpy()
    return out


def _forward(qpb, H, f, A, b, meq, **kw):
    sol = qpb.solve_eq(_dev(H), _dev(f), _dev(A), _dev(b), meq, **kw)
    torch.cuda.synchronize()
    return sol.x.cpu().numpy(), sol.lam.cpu().numpy(), sol.active.cpu().numpy(), sol.status.cpu().numpy()


def _words(mask):
    Bq, m = mask.shape
    act = np.zeros((Bq, (m + 31) // 32), np.uint32)
    for i, j in zip(*np.nonzero(mask)):
        act[i, j // 32] |= np.uint32(1) << np.uint32(j % 32)
    return act.view(np.int32)


_CASES = {}


def _case(qpb, n, m, meq):
    """One shape's inputs, its forward on the GPU, the two cotangents and the
    oracle's gradients: computed once, shared, never modified."""
    key = (n, m, meq)
    if key not in _CASES:
        H, f, A, b, xc = KO.family(SEED, B, n, m, meq)
        x, lam, act, st = _forward(qpb, H, f, A, b, meq)
        assert (st == OK).all(), st
        mask = qpb.active_mask_to_bool(act, m)
        rng = np.random.default_rng([SEED, n, m, meq, 2])
        g, gl = rng.standard_normal((B, n)), rng.standard_normal((B, m))
        ref = [DO.backward(H[i], x[i], lam[i], A[i], mask[i], g[i], gl[i]) for i in range(B)]
        ref = {k: np.array([r[j] for r in ref]) for j, k in enumerate(NAMES)}
        _CASES[key] = dict(H=H, f=f, A=A, b=b, x=x, lam=lam, act=act, st=st, mask=mask, g=g, gl=gl, ref=ref)
    return _CASES[key]


def _run(qpb, c, **kw):
    return _dual(qpb, kw.pop("shared", 0), c["H"], c["A"], c["x"], c["lam"], c["act"], kw.pop("st", c["st"]),
                 kw.pop("g", c["g"]), kw.pop("gl", c["gl"]), **kw)


# ------------------------------------------------------- 1. parity and certificate
@pytest.mark.parametrize("n,m,meq", DENSE_SHAPES + WAVE_SHAPES)
def test_parity_and_certificate(qpb, n, m, meq):
    c = _case(qpb, n, m, meq)
    out = _run(qpb, c)
    assert set(out) == set(NAMES)
    errs = {k: float(_rel(out[k], c["ref"][k]).max()) for k in NAMES}
    cert = np.array([DO.certificate(c["H"][i], c["A"][i], c["mask"][i], c["g"][i], c["gl"][i], out["f"][i],
                                    out["b"][i]) for i in range(B)])
    print(f"({n},{m},{meq}): active rows {c['mask'].sum(axis=1).min()}..{c['mask'].sum(axis=1).max()} "
          f"errors {errs} certificate stat {cert[:, 0].max():.2e} prim {cert[:, 1].max():.2e}")
    for k in NAMES:
        assert np.isfinite(out[k]).all(), k
        assert errs[k] <= X_TOL, (k, errs[k])
    assert cert.max() <= KKT_TOL, cert.max(axis=0)
    assert np.array_equal(out["H"], out["H"].transpose(0, 2, 1))
    assert (out["A"][~c["mask"]] == 0.0).all() and (out["b"][~c["mask"]] == 0.0).all()
    # the cotangent on lam is not a no-op: the outputs differ from qpb_solve_backward's
    assert not np.array_equal(out["f"], _run(qpb, c, gl=None)["f"])
    # the Python call returns the same bits
    sol = qpb.Solution(_dev(c["x"]), _dev(c["lam"]), _dev(c["act"]), _dev(c["st"]), None)
    got = qpb.solve_backward_dual(_dev(c["H"]), _dev(c["A"]), sol, _dev(c["g"]), _dev(c["gl"]))
    torch.cuda.synchronize()
    assert _same(out, {k: t.cpu().numpy() for k, t in zip(NAMES, got)})


# ------------------------------------------------------- 2. glam NULL is qpb_solve_shared_backward
@pytest.mark.parametrize("n,m,meq", PATH_SHAPES)
@pytest.mark.parametrize("shared", [0, 1, 2, 3])
def test_null_glam_is_the_shared_backward_bit_for_bit(qpb, n, m, meq, shared):
    c = _shared_case(qpb, n, m, meq)
    H, A = SC.operand(c["H0"], B, shared & 1), SC.operand(c["A0"], B, shared & 2)
    ref = SC.shared_backward(qpb, shared, H, A, c["x"], c["lam"], c["act"], c["st"], c["g"])
    got = _dual(qpb, shared, H, A, c["x"], c["lam"], c["act"], c["st"], c["g"], None)
    assert _same(got, ref)
    if shared == 0:
        assert _same(got, _plain_backward(qpb, H, A, c["x"], c["lam"], c["act"], c["st"], c["g"]))


# ------------------------------------------------------- 3. linearity: the columns of the lower block
@pytest.mark.parametrize("n,m,meq", PATH_SHAPES)
def test_unit_glam_gives_a_column_of_the_inverse(qpb, n, m, meq):
    """gx = 0 and glam = e_i on an active row i: dx and dlam are minus column
    n + pos(i) of K^{-1}.  One QP, every active row of it as a batch."""
    c = _case(qpb, n, m, meq)
    q = 5
    rows = np.flatnonzero(c["mask"][q])
    assert len(rows) >= 2
    k = len(rows)
    rep = lambda a: np.broadcast_to(a[q], (k,) + a[q].shape).copy()  # noqa: E731
    gl = np.zeros((k, m))
    gl[np.arange(k), rows] = 1.0
    out = _dual(qpb, 0, rep(c["H"]), rep(c["A"]), rep(c["x"]), rep(c["lam"]), rep(c["act"]), rep(c["st"]),
                np.zeros((k, n)), gl)
    for j in range(k):
        ref = DO.backward(c["H"][q], c["x"][q], c["lam"][q], c["A"][q], c["mask"][q], np.zeros(n), gl[j])
        for name, r in zip(NAMES, ref):
            assert _rel(out[name][j][None], r[None])[0] <= X_TOL, (j, name)
    # ... and the block is symmetric, d lam_i / d(glam_j) = d lam_j / d(glam_i): two entries, each within the bar
    S = -out["b"][:, rows]
    assert np.abs(S - S.T).max() <= 2 * X_TOL * (1.0 + np.abs(S).max())


# ------------------------------------------------------- 4. glam is ignored where it must be
@pytest.mark.parametrize("n,m,meq", PATH_SHAPES)
def test_glam_outside_w_and_of_failed_qps_is_ignored(qpb, n, m, meq):
    c = _case(qpb, n, m, meq)
    H = c["H"].copy()
    H[3] = -np.eye(n)
    x, lam, act, st = _forward(qpb, H, c["f"], c["A"], c["b"], meq)
    assert ((st == NOT_SPD) == (np.arange(B) == 3)).all(), st
    x1, lam1, act1, st1 = _forward(qpb, H, c["f"], c["A"], c["b"], meq, max_iter=1)
    capped = np.flatnonzero(st1 == MAX_ITER)[::6]  # (one iteration caps most of the batch: a sixth of them)
    assert len(capped) > 0
    for a, a1 in ((x, x1), (lam, lam1), (act, act1), (st, st1)):
        a[capped] = a1[capped]
    nanx = np.flatnonzero(st == OK)[[4, 20]]
    st[nanx] = NUMERICAL
    x[nanx] = np.nan
    lam[nanx] = np.nan
    bad = st != OK
    assert {MAX_ITER, NOT_SPD, NUMERICAL} <= set(st.tolist()) and (~bad).sum() > B // 2
    mask = qpb.active_mask_to_bool(act, m)
    ignored = ~mask | bad[:, None]
    clean, poisoned = np.where(ignored, 0.0, c["gl"]), np.where(ignored, np.nan, c["gl"])
    ref = _dual(qpb, 0, H, c["A"], x, lam, act, st, c["g"], clean)
    got = _dual(qpb, 0, H, c["A"], x, lam, act, st, c["g"], poisoned)
    assert _same(got, ref)
    for k in NAMES:
        assert (got[k][bad] == 0.0).all(), k
        assert np.isfinite(got[k]).all(), k
    # with a shared H and A the failed QPs contribute exactly 0: the sums equal those without their glam
    c3 = _shared_case(qpb, n, m, meq)
    st3, x3, lam3 = c3["st"].copy(), c3["x"].copy(), c3["lam"].copy()
    st3[::7], x3[::7], lam3[::7] = MAX_ITER, np.nan, np.nan
    ign3 = ~c3["mask"] | (st3 != OK)[:, None]
    ref3 = _dual(qpb, 3, c3["H0"], c3["A0"], x3, lam3, c3["act"], st3, c3["g"], np.where(ign3, 0.0, c3["gl"]))
    got3 = _dual(qpb, 3, c3["H0"], c3["A0"], x3, lam3, c3["act"], st3, c3["g"], np.where(ign3, np.nan, c3["gl"]))
    assert _same(got3, ref3) and all(np.isfinite(v).all() for v in got3.values())


# ------------------------------------------------------- 5. NULL outputs, NULL status
@pytest.mark.parametrize("n,m,meq", PATH_SHAPES)
def test_every_need_subset_and_null_status(qpb, n, m, meq):
    c = _case(qpb, n, m, meq)
    full = _run(qpb, c)
    for r in range(1, 4):
        for need in itertools.combinations(NAMES, r):
            assert _same(_run(qpb, c, need=need), {k: full[k] for k in need}), need
    assert _same(_run(qpb, c, st=None), full)
    # the Python call: what is left out of `need` comes back as None
    sol = qpb.Solution(_dev(c["x"]), _dev(c["lam"]), _dev(c["act"]), None, None)
    gH, gf, gA, gb = qpb.solve_backward_dual(_dev(c["H"]), _dev(c["A"]), sol, _dev(c["g"]), _dev(c["gl"]),
                                             need=("f", "b"))
    torch.cuda.synchronize()
    assert gH is None and gA is None
    assert _same({"f": gf.cpu().numpy(), "b": gb.cpu().numpy()}, {"f": full["f"], "b": full["b"]})


# ------------------------------------------------------- 6. rows the orthogonalisation skips
@pytest.mark.parametrize("n,m,meq", PATH_SHAPES)
@pytest.mark.parametrize("how", ["duplicate_later", "duplicate_earlier", "overfull"])
def test_a_skipped_rows_glam_is_ignored(qpb, n, m, meq, how):
    """A hand-made mask.  duplicate: row j2 is made a copy of the active row j1
    and marked active; in row order the second of the two is dependent.
    overfull: every row is marked, |W| = m > n, and the rows met after n
    independent ones are skipped.  A skipped row has dlam = 0 (gb = 0,
    gA = lam dx^T), its glam -- NaN here -- is ignored, and everything else is
    the system on the kept rows."""
    c = _case(qpb, n, m, meq)
    Bq = 8
    A, lam, mask = c["A"][:Bq].copy(), c["lam"][:Bq].copy(), c["mask"][:Bq].copy()
    gl = c["gl"][:Bq].copy()
    skipped = np.zeros((Bq, m), bool)
    for i in range(Bq):
        if how == "overfull":
            lam[i, ~mask[i]] = 0.37
            mask[i] = True
            skipped[i, n:] = True  # generic rows: the first n are independent
            continue
        on, off = np.flatnonzero(mask[i]), np.flatnonzero(~mask[i])
        j1 = on[len(on) // 2]
        cand = off[off > j1] if how == "duplicate_later" else off[off < j1]
        if len(cand) == 0:  # no inactive row on that side: the other one
            cand = off
        j2 = cand[0]
        A[i, j2] = A[i, j1]
        lam[i, j2] = 0.37
        mask[i, j2] = True
        skipped[i, max(j1, j2)] = True
    gl[skipped] = np.nan
    out = _dual(qpb, 0, c["H"][:Bq], A, c["x"][:Bq], lam, _words(mask), c["st"][:Bq], c["g"][:Bq], gl)
    for i in range(Bq):
        keep = mask[i] & ~skipped[i]
        gH, gf, gA, gb = DO.backward(c["H"][i], c["x"][i], lam[i], A[i], keep, c["g"][i], gl[i])
        gA[skipped[i]] = np.outer(lam[i, skipped[i]], gf)
        for k, ref in zip(NAMES, (gH, gf, gA, gb)):
            assert np.isfinite(out[k][i]).all(), (i, k)
            assert _rel(out[k][i][None], ref[None])[0] <= X_TOL, (i, k)
        assert (out["b"][i, skipped[i]] == 0.0).all()
        assert (out["A"][i][~mask[i]] == 0.0).all() and (out["b"][i][~mask[i]] == 0.0).all()


# ------------------------------------------------------- 7. shared operands
_SHARED = {}


def _shared_case(qpb, n, m, meq):
    """ONE H0 and A0 for the batch (tests/shared_cases.py), the forward on the
    GPU, the cotangents, and the unshared dual backward on copies: once, shared."""
    key = (n, m, meq)
    if key not in _SHARED:
        H0, f, A0, b = SC.family(B, n, m, meq)
        sol = qpb.solve_shared(_dev(H0), _dev(f), _dev(A0), _dev(b), meq)
        torch.cuda.synchronize()
        x, lam, act, st = (t.cpu().numpy() for t in (sol.x, sol.lam, sol.active, sol.status))
        assert (st == OK).all(), st
        rng = np.random.default_rng([SC.SEED, B, n, m, meq, 2])
        g, gl = rng.standard_normal((B, n)), rng.standard_normal((B, m))
        ref = _dual(qpb, 0, SC.expand(H0, B), SC.expand(A0, B), x, lam, act, st, g, gl)
        _SHARED[key] = dict(H0=H0, A0=A0, x=x, lam=lam, act=act, st=st, g=g, gl=gl, ref=ref,
                            mask=qpb.active_mask_to_bool(act, m))
    return _SHARED[key]


def _bits(a, b):
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("n,m,meq", [(16, 32, 4), (20, 40, 4)])
def test_shared_operands(qpb, n, m, meq):
    c = _shared_case(qpb, n, m, meq)
    ref = c["ref"]
    bounds = SC.sum_bound(c["x"], ref["f"], ref["b"], c["lam"], c["mask"], np.ones(B, bool))
    worst = 0.0
    for shared in (1, 2, 3):
        args = (shared, SC.operand(c["H0"], B, shared & 1), SC.operand(c["A0"], B, shared & 2), c["x"], c["lam"],
                c["act"], c["st"], c["g"], c["gl"])
        got = _dual(qpb, *args)
        assert got.keys() == ref.keys()
        for k in got:
            summed = (k == "H" and shared & 1) or (k == "A" and shared & 2)
            if not summed:
                assert _bits(got[k], ref[k]), (shared, k, "per-QP output differs")
                continue
            bound = bounds[0] if k == "H" else bounds[1]
            delta = np.abs(got[k] - SC.fsum0(ref[k]))
            assert np.isfinite(got[k]).all() and (delta <= bound).all(), (shared, k, float((delta - bound).max()))
            worst = max(worst, float(np.where(bound > 0, delta / np.where(bound > 0, bound, 1.0), 0.0).max()))
            if k == "H":
                assert _bits(got[k], np.ascontiguousarray(got[k].T)), (shared, "gH is not symmetric bit for bit")
        # the same call twice, and on a side stream: the same bits
        assert _same(_dual(qpb, *args), got)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        assert _same(_dual(qpb, *args, stream=side), got)
        qpb.release_stream_workspace(side)
    print(f"n={n} m={m}: worst |delta| / bound of a summed gradient {worst:.3g}")
    # the Python call with a 2-D H and A
    sol = qpb.Solution(_dev(c["x"]), _dev(c["lam"]), _dev(c["act"]), _dev(c["st"]), None)
    gH, gf, gA, gb = qpb.solve_backward_dual(_dev(c["H0"]), _dev(c["A0"]), sol, _dev(c["g"]), _dev(c["gl"]))
    torch.cuda.synchronize()
    assert gH.shape == (n, n) and gA.shape == (m, n) and _bits(gf.cpu().numpy(), ref["f"])


# ------------------------------------------------------- 8. independence
@pytest.mark.parametrize("n,m,meq", PATH_SHAPES)
def test_a_qp_depends_on_its_own_inputs_only(qpb, n, m, meq):
    c = _case(qpb, n, m, meq)
    full = _run(qpb, c)
    perm = np.random.default_rng(SEED).permutation(B)
    got = _dual(qpb, 0, c["H"][perm], c["A"][perm], c["x"][perm], c["lam"][perm], c["act"][perm], c["st"][perm],
                c["g"][perm], c["gl"][perm])
    assert _same(got, {k: v[perm] for k, v in full.items()})
    one = slice(5, 6)
    alone = _dual(qpb, 0, c["H"][one], c["A"][one], c["x"][one], c["lam"][one], c["act"][one], c["st"][one],
                  c["g"][one], c["gl"][one])
    assert _same(alone, {k: v[one] for k, v in full.items()})


def test_above_the_wave_class_is_unsupported(qpb):
    n, Bq = 33, 2
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    sol = qpb.Solution(z(Bq, n), None, None, None, None)
    with pytest.raises(qpb.QPBError) as e:
        qpb.solve_backward_dual(z(Bq, n, n), None, sol, z(Bq, n), None)
    assert e.value.code == qpb.ERR_UNSUPPORTED and "n<=32" in str(e.value)
