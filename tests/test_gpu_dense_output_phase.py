"""The output phase of gi_dense (csrc/qpb_gi.hip, after the active-set loop):
the gather of the active rows of A in two groups of eight, g = f + A_W^T lam,
row16::solve_x, and the stores of x, lam, the active words and the status --
on every form of gi_group, and on solve_x's other users.

The cases plant the FINAL active set (tests/planted.py's integer construction:
x*, lam* > 0 on k independent tight rows, integer slack >= 1 elsewhere, so the
active set is unique and strictly complementary) and compare with a dense
numpy solve of the KKT system on that set (tests/kkt_oracle.py) at
tests/test_gpu_positions.py's tolerance, 1e-9 relative: the data are integers
with cond(H) < 12 and |x*| <= 3, so fp64 leaves five orders of margin.  The
mask is compared bit for bit.  Where an entry point has a bitwise sibling
(qpb_solve_shared on a 2-D A against qpb_solve on copies; a QP alone or in a
batch of four against the same QP in another batch) equality is exact.
qpb_solve_factored is held to its own contract (qpb.h: status and active set
those of qpb_solve_shared, x and lam within rounding), i.e. the tolerance.

solve_x's other users, qpb_solve_box and qpb_solve_box_backward at n = 16, are
held bit for bit to tests/golden/gi_dense_v118_solve_x.npz, recorded by
tools/record_solve_x_golden.py on the commit before gi_dense's output solves
became row16::solve_x_frozen (the box kernels keep solve_x).

A drop cannot be planted, so the drop / re-add cases come from a numpy model
of the kernel's iteration (`_gi_trace`: Goldfarb-Idnani with the kernel's
selection rule, after tools/gi_select_sim.py) run over seeded random QPs until
one shows the history wanted; the test asserts the history on the model, and
that the GPU took as many trips and ended on the same set.
"""
import os

import numpy as np
import pytest

import kkt_oracle as KO
import planted as P

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

X_TOL = 1e-9  # tests/test_gpu_positions.py
OK, MAX_ITER, NOT_SPD, INFEASIBLE, NUMERICAL = 0, 1, 2, 3, 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gi_dense_v118_solve_x.npz")


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda() for a in arrays]


def _host(sol):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in sol]


def _same(a, b):
    return all(np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip(a, b))


# ------------------------------------------------------------------ the cases
def _planted(n, m, k, seed, meq=0, H=None, A=None):
    """One QP whose final active set is rows 0 .. meq-1 (equalities, multipliers
    of both signs) and k inequality rows at random indices, lam* in [1, 4] on
    them; the meq + k rows are independent.  H and / or A given: shared ones
    (A's rows must then be independent on every subset drawn: checked)."""
    rs = np.random.default_rng([seed, n, m, k, meq])
    H = P._spd(rs, n) if H is None else H
    x = rs.integers(-3, 4, n).astype(np.float64)
    tight = np.zeros(m, bool)
    tight[:meq] = True
    tight[meq + rs.permutation(m - meq)[:k]] = True
    if A is None:
        A = P._rows(rs, m, n)
        if meq + k:
            A[tight] = P._independent_rows(rs, meq + k, n)
    assert meq + k == 0 or np.linalg.matrix_rank(A[tight]) == meq + k
    lam = np.zeros(m)
    lam[tight] = P._mult(rs, meq + k)
    lam[:meq] *= np.where(np.arange(meq) % 2 == 0, 1.0, -1.0)
    b = A @ x + np.where(tight, 0.0, rs.integers(1, 6, m))
    f = -H @ x - A.T @ lam
    return H, f, A, b, x, lam, tight


def _batch(n, m, sizes, seed, **kw):
    qs = [_planted(n, m, k, seed + i, **kw) for i, k in enumerate(sizes)]
    return [np.stack(v) for v in zip(*qs)]


def _kkt_ref(H, f, A, rhs, act):
    """x and lam of min 1/2 x H x + f x s.t. A[act] x = rhs[act], through
    kkt_oracle.backward's dense solve: with xs any point on the rows and
    g = H xs + f, its (dx, dlam) are x - xs and lam."""
    W = np.flatnonzero(act)
    xs = np.linalg.lstsq(A[W], rhs[W], rcond=None)[0] if len(W) else np.zeros(len(f))
    _, dx, _, gb = KO.backward(H, xs, None, A, act, H @ xs + f)
    return xs + dx, -gb


def _check(qpb, sol, H, f, A, rhs, tight, what, meq=0, signed=False):
    """status OK, mask == tight bit for bit, x and lam within X_TOL of the KKT
    solve on the planted set, lam == 0 off the set and > 0 on its inequalities."""
    x, lam, act, st = sol[0], sol[1], sol[2], sol[-2]
    B, m = rhs.shape
    mask = qpb.active_mask_to_bool(act, m)
    assert (st == OK).all(), (what, st)
    assert np.array_equal(mask, tight), (what, np.nonzero((mask != tight).any(axis=1))[0])
    ex = el = 0.0
    for i in range(B):
        Hi, Ai = (H if H.ndim == 2 else H[i]), (A if A.ndim == 2 else A[i])
        xr, lr = _kkt_ref(Hi, f[i], Ai, rhs[i], tight[i])
        ex = max(ex, np.abs(x[i] - xr).max() / max(1.0, np.abs(xr).max()))
        el = max(el, np.abs(lam[i] - lr).max() / max(1.0, np.abs(lr).max()))
    print(f"{what}: {B} QPs, set sizes {tight.sum(axis=1).tolist()}, x err {ex:.2e}, lam err {el:.2e}, "
          f"iters {sol[-1].tolist()}")
    assert ex <= X_TOL and el <= X_TOL, (what, ex, el)
    assert (lam[~mask] == 0.0).all(), what
    if not signed:
        assert (lam[:, meq:][mask[:, meq:]] > 0.0).all(), what


# ------------------------------------------------- final active-set sizes (FULL)
SIZES = [0] * 4 + [1] * 4 + [8] * 4 + [9] * 4 + [15] * 4 + [16] * 4 + [0, 1, 9, 16] + [16, 8, 0, 15]


def test_final_set_sizes(qpb):
    """n = 16, m = 32: whole waves at 0 (no gather), 1, 8 and 9 (the second
    load group empty, then holding one row), 15 and 16 (every position), and
    waves that mix 0, 1, 9, 16 and 16, 8, 0, 15, where the wave-uniform group
    tests cover rows the smaller QPs do not have."""
    H, f, A, b, xs, lams, tight = _batch(16, 32, SIZES, 1180)
    sol = _host(qpb.solve(*_dev(H, f, A, b)))
    _check(qpb, sol, H, f, A, b, tight, "sizes")
    ex = np.abs(sol[0] - xs).max()
    assert ex <= X_TOL * 3.0, ex  # the planted x* itself, |x*| <= 3
    assert (sol[4] >= tight.sum(axis=1) + 1).all()


# ----------------------------------------------------------- drops and re-adds
def _gi_trace(H, f, A, b):
    """Goldfarb-Idnani as the kernel runs it (D = A L^-T, Householder on an
    ADD, Givens on a DROP, the violated row of the largest -s / |D[r, q:]|),
    in numpy.  Returns (trips, events, final set): events are ('add', row) and
    ('drop', row) in order; trips counts them."""
    n, m = len(f), len(b)
    L = np.linalg.cholesky(H)
    Dc = np.linalg.solve(L, A.T).T
    s = b + Dc @ np.linalg.solve(L, f)
    an = np.linalg.norm(A, axis=1)
    W, R, lam, ev = [], np.zeros((0, 0)), np.zeros(0), []
    while len(ev) < 200:
        q = len(W)
        act = np.zeros(m, bool)
        act[W] = True
        viol = ~act & (s < -1e-9 * (an + np.abs(b)))
        if not viol.any():
            return len(ev), ev, sorted(W)
        fn = np.linalg.norm(Dc[:, q:], axis=1)
        p = int(np.argmax(np.where(viol, -s / np.where(fn > 0, fn, np.inf), -np.inf)))
        up = 0.0
        while True:
            q = len(W)
            d = Dc[p]
            d1, d2 = -d[:q], d[q:]
            r = np.linalg.solve(R, d1) if q else np.zeros(0)
            cand = [(lam[j] / r[j], j) for j in range(q) if r[j] > 0]
            t1, k = min(cand) if cand else (np.inf, -1)
            nd2 = d2 @ d2
            t2 = -s[p] / nd2 if nd2 > 1e-24 * (d @ d) else np.inf
            t = min(t1, t2)
            if not np.isfinite(t):
                return len(ev), ev, None
            if np.isfinite(t2):
                s = s + t * (Dc[:, q:] @ d2)
            lam = lam - t * r
            up += t
            if t2 <= t1:
                ev.append(("add", p))
                nrm = np.sqrt(nd2)
                alpha = -nrm if d2[0] <= 0 else nrm
                v = d2.copy()
                v[0] += alpha
                Dc[:, q:] -= np.outer(Dc[:, q:] @ v, v) * (2 / (v @ v))
                Rn = np.zeros((q + 1, q + 1))
                Rn[:q, :q], Rn[:q, q], Rn[q, q] = R, d1, alpha
                R, lam = Rn, np.append(lam, up)
                W.append(p)
                break
            ev.append(("drop", W[k]))
            W.pop(k)
            lam = np.delete(lam, k)
            R = np.delete(R, k, axis=1)
            for j in range(k, q - 1):
                h = np.hypot(R[j, j], R[j + 1, j])
                c, sn = R[j, j] / h, R[j + 1, j] / h
                G = np.array([[c, sn], [-sn, c]])
                R[[j, j + 1], :] = G @ R[[j, j + 1], :]
                Dc[:, [j, j + 1]] = Dc[:, [j, j + 1]] @ G.T
            R = R[:q - 1, :]
    return len(ev), ev, None


def _random_qp(seed, n=16, m=32):
    """A dense QP with many violated rows at the unconstrained minimiser."""
    rs = np.random.default_rng([seed, n, m])
    M = rs.standard_normal((n, n))
    H = np.eye(n) + M.T @ M / n
    f = 3.0 * rs.standard_normal(n)
    A = rs.standard_normal((m, n))
    A /= np.linalg.norm(A, axis=1, keepdims=True)
    b = A @ np.linalg.solve(H, -f) + rs.uniform(-1.5, 1.0, m)
    return H, f, A, b


def _history(ev, final):
    """(rows dropped and absent at the end; rows dropped, added again and present at the end)"""
    dropped, readded = set(), set()
    for kind, row in ev:
        if kind == "drop":
            dropped.add(row)
        elif row in dropped:
            readded.add(row)
    return {r for r in dropped if r not in final}, {r for r in readded if r in final}


DROP_SEED, READD_SEED = 3, 0  # the first seeds of _random_qp with the two histories (test_drop_and_readd)


def test_drop_and_readd(qpb):
    """Two QPs in one wave with two planted partners.  The first (seed
    DROP_SEED) adds a row, drops it and ends without it: the row's line was
    asked for but is not gathered.  The second (seed READD_SEED) drops a row
    and adds it again: gathered at its second position.  The seeds are the
    first of `_random_qp` with those histories in `_gi_trace` (asserted here);
    the GPU must take trips + 1 iterations (the last finds no violated row)
    and end on the model's set, and meet the KKT solve on it."""
    qa, qb = _random_qp(DROP_SEED), _random_qp(READD_SEED)
    ta, ea, Wa = _gi_trace(*qa)
    tb, eb, Wb = _gi_trace(*qb)
    assert Wa is not None and _history(ea, Wa)[0], ea
    assert Wb is not None and _history(eb, Wb)[1], eb
    p0, p1 = _planted(16, 32, 9, 1181), _planted(16, 32, 16, 1182)
    H, f, A, b = (np.stack(v) for v in zip(qa, p0[:4], qb, p1[:4]))
    tight = np.zeros((4, 32), bool)
    tight[0, Wa], tight[2, Wb] = True, True
    tight[1], tight[3] = p0[6], p1[6]
    sol = _host(qpb.solve(*_dev(H, f, A, b)))
    print(f"drop: {ea}\nre-add: {eb}")
    _check(qpb, sol, H, f, A, b, tight, "drop / re-add")
    assert sol[4][0] == ta + 1 and sol[4][2] == tb + 1, (sol[4], ta, tb)


# ------------------------------------------------------------- ragged batches
@pytest.mark.parametrize("n,m", [(16, 32), (13, 26)])
def test_ragged_batches(qpb, n, m):
    """B = 1, 2, 3, 5, 7: the rows past the batch's end replay the last QP and
    store nothing.  Every QP is bitwise what it is in a batch of four (QPs
    0..3 and 4..7 solved as two launches), and the outputs' allocations past B
    keep their fill."""
    sizes = [9, 0, min(16, n), 1, 8, min(15, n - 1), 2, 9]
    H, f, A, b, _, _, tight = _batch(n, m, sizes, 1183)
    four = [_host(qpb.solve(*_dev(H[i:i + 4], f[i:i + 4], A[i:i + 4], b[i:i + 4]))) for i in (0, 4)]
    ref = [np.concatenate([four[0][k], four[1][k]]) for k in range(5)]
    _check(qpb, ref, H, f, A, b, tight, f"batches of four n={n}")
    for B in (1, 2, 3, 5, 7):
        out = qpb._empty_solution(8, n, m, torch.device("cuda", 0))
        for t in out:
            t.view(torch.uint8).fill_(0xA5)
        view = type(out)(*(t[:B] for t in out))
        qpb.solve(*_dev(H[:B], f[:B], A[:B], b[:B]), out=view)
        got = _host(out)
        assert _same([g[:B] for g in got], [r[:B] for r in ref]), B
        assert all((g[B:].view(np.uint8) == 0xA5).all() for g in got), B


# --------------------------------------------------------------- padded forms
@pytest.mark.parametrize("n,m", [(13, 26), (16, 20)])
def test_padded_forms(qpb, n, m):
    """The non-N16 form (n = 13: column clamp) and the non-FULL one (m = 20:
    row clamp), with sets up to n and a last wave of three."""
    sizes = [0, 1, 9, n, 8, n - 1, 9, 2, n, 0, 1]
    H, f, A, b, _, _, tight = _batch(n, m, sizes, 1184)
    sol = _host(qpb.solve(*_dev(H, f, A, b)))
    _check(qpb, sol, H, f, A, b, tight, f"padded n={n} m={m}")


# ---------------------------------------------------- other forms of gi_group
def test_eq_form(qpb):
    """qpb_solve_eq, meq = 2: positions 0 and 1 are the equalities."""
    sizes = [0, 7, 14, 1, 9, 6]
    H, f, A, b, _, _, tight = _batch(16, 32, sizes, 1185, meq=2)
    sol = _host(qpb.solve_eq(*_dev(H, f, A, b), 2))
    _check(qpb, sol, H, f, A, b, tight, "eq", meq=2)


def test_range_form(qpb):
    """qpb_solve_range: in every QP the tight rows at odd indices are held at
    their LOWER side (the row negated, bl = -b, no upper side or a loose one);
    lam is <= 0 there and the `lower` word marks them."""
    sizes = [9, 1, 16, 8, 0]
    H, f, A, b, _, _, tight = _batch(16, 32, sizes, 1186)
    low = tight & (np.arange(32) % 2 == 1)[None, :]
    A2 = np.where(low[:, :, None], -A, A)
    bu = np.where(low, np.where(np.arange(32) % 4 == 1, np.inf, -b + 7.0), b)
    bl = np.where(low, -b, b - 20.0)
    rhs = np.where(low, bl, bu)
    sol = _host(qpb.solve_range(*_dev(H, f, A2, bl, bu)))
    _check(qpb, sol, H, f, A2, rhs, tight, "range", signed=True)
    assert np.array_equal(qpb.active_mask_to_bool(sol[3], 32), low)
    assert (sol[1][low] < 0.0).all() and (sol[1][tight & ~low] > 0.0).all()


def _shared_case(seed, sizes):
    rs = np.random.default_rng(seed)
    H = P._spd(rs, 16)
    while True:
        A = P._rows(rs, 32, 16)
        try:
            qs = [_planted(16, 32, k, seed + i, H=H, A=A) for i, k in enumerate(sizes)]
            break
        except AssertionError:
            continue
    f, b, tight = (np.stack([q[j] for q in qs]) for j in (1, 3, 6))
    return H, A, f, b, tight


def test_shared_and_factored_forms(qpb):
    """qpb_solve_shared with a 2-D H and a 2-D A (the QP stride of A is
    strideA = 0, not m n): bitwise qpb_solve on copies.  qpb_solve_factored
    (FM = 2) on the same case: status and active set those of the shared
    solve, x and lam within the tolerance."""
    sizes = [9, 0, 16, 1, 8, 12]
    H, A, f, b, tight = _shared_case(1187, sizes)
    B = len(sizes)
    Ht, At = np.broadcast_to(H, (B, 16, 16)).copy(), np.broadcast_to(A, (B, 32, 16)).copy()
    plain = _host(qpb.solve(*_dev(Ht, f, At, b)))
    Hd, Ad, fd, bd = _dev(H, A, f, b)
    shared = _host(qpb.solve_shared(Hd, fd, Ad, bd))
    assert _same(shared, plain)
    _check(qpb, shared, H, f, A, b, tight, "shared 2-D")
    half = _host(qpb.solve_shared(_dev(Ht)[0], fd, Ad, bd))  # batched H, shared A
    assert _same(half, plain)
    F = qpb.factor_shared(Hd, Ad)
    fact = _host(qpb.solve_factored(F, fd, bd))
    assert int(F.status.cpu()[0]) == OK
    _check(qpb, fact, H, f, A, b, tight, "factored")
    assert np.array_equal(fact[2], shared[2]) and np.array_equal(fact[3], shared[3])


# ------------------------------------------------------- solve_x's other users
def test_box_users_of_solve_x_golden(qpb):
    """qpb_solve_box and qpb_solve_box_backward at n = 16, 64 QPs: every output
    bit for bit the recorded one."""
    g = np.load(GOLDEN)
    H, f, lb, ub, gx = _dev(*(g[k] for k in ("H", "f", "lb", "ub", "gx")))
    sol = qpb.solve_box(H, f, lb, ub)
    grads = qpb.solve_box_backward(H, sol, gx)
    torch.cuda.synchronize()
    for k in ("x", "lam", "active", "status", "iters"):
        got = getattr(sol, k).cpu().numpy()
        assert np.array_equal(got.view(np.uint8), g[k].view(np.uint8)), k
    for k, t in zip(("gH", "gf", "glb", "gub"), grads):
        assert np.array_equal(t.cpu().numpy().view(np.uint8), g[k].view(np.uint8)), k
    nact = qpb.active_mask_to_bool(g["active"], 32).sum(axis=1)
    assert nact.min() <= 4 and nact.max() >= 12 and (g["status"] == OK).all()  # small and large sets are recorded


# ----------------------------------------------------------------- status paths
def test_status_paths(qpb):
    """One wave: a healthy QP, -H (QPB_NOT_SPD), two contradicting rows
    (x_0 <= -1 and -x_0 <= -1: QPB_INFEASIBLE, found by the iteration) and a
    NaN in A (QPB_NUMERICAL).  tests/test_gpu_status_contract.py's contract:
    the set-up failures ran no iteration and hold lam = 0 and an empty set; the
    infeasible QP holds its dual iterate -- x and lam finite, lam >= 0 and 0
    off the set, |H x + f + A^T lam| within 1e-9; the healthy QP is bitwise
    what it is alone."""
    H, f, A, b, _, _, tight = _batch(16, 32, [9, 9, 0, 9], 1188)
    H[1] = -H[1]
    A[2, 5], b[2, 5] = np.eye(16)[0], -1.0
    A[2, 20], b[2, 20] = -np.eye(16)[0], -1.0
    A[3, 17, 3] = np.nan
    x, lam, act, st, it = sol = _host(qpb.solve(*_dev(H, f, A, b)))
    print(f"status {st.tolist()} iters {it.tolist()}")
    assert st.tolist() == [OK, NOT_SPD, INFEASIBLE, NUMERICAL], st
    mask = qpb.active_mask_to_bool(act, 32)
    for i in (1, 3):
        assert it[i] == 0 and (lam[i] == 0).all() and not mask[i].any(), i
    assert it[2] >= 1 and np.isfinite(x[2]).all() and np.isfinite(lam[2]).all()
    assert (lam[2] >= 0).all() and (lam[2][~mask[2]] == 0).all()
    r = H[2] @ x[2] + f[2] + A[2].T @ lam[2]
    scale = 1.0 + np.abs(f[2]).max() + np.abs(H[2]).sum(axis=1).max() * np.abs(x[2]).max()
    assert np.abs(r).max() <= 1e-9 * scale, np.abs(r).max() / scale
    alone = _host(qpb.solve(*_dev(H[:1], f[:1], A[:1], b[:1])))
    assert _same([v[:1] for v in sol], alone)
    _check(qpb, alone, H[:1], f[:1], A[:1], b[:1], tight[:1], "healthy")
