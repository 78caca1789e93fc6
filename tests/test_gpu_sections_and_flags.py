"""The diagnostic builds and flags of qpb.h, and qpb_qf_eval.

a. qpb_solve_sections: its three stamped kernel builds (n = 16 with
   16 < m <= 32; the wavefront class; the Gram class) solve like qpb_solve and
   account their ticks as qpb.h says: into rows < number of workgroups of a
   256 x 20 buffer, added, never outside it; and its argument checks.
b. QPB_FLAG_DIAG_L2 / QPB_FLAG_DIAG_MALL alias the inputs inside
   gi_dense_kernel only; the retired flags 4, 8 and 128 are accepted and
   ignored; qpb_solve_box's flags select nothing.
c. qpb_qf_eval against the same expression in numpy.longdouble, within the
   rounding-error bound of the kernel's own summation.

"Equal" is bitwise over every output array (_same)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_status_contract import _check_parity, _dev, _host, _oracle, _same  # noqa: E402

FILL = 0xA5
SECTIONS_LEN = 256 * 20  # QPB_SECTIONS_LEN
GUARD_WORDS = 64
GUARD_VALUE = 0x5A5A5A5A5A5A5A5A
FLAG_DIAG_L2, FLAG_DIAG_MALL, FLAG_DIAG_WAVE = 1, 16, 256
RETIRED = [4, 8, 128, 4 | 8 | 128]


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


# ------------------------------------------------------------- a. stamped builds
# (build, n, m, batch); the section indices each build stamps (clk.tick in
# qpb_gi.hip -- "substitution", index 2, is folded into the sweep --,
# qpb_gi_wave.hip, qpb_gi_gram.hip) and its workgroups and stamping waves
STAMPED = [("n16", 16, 20, 37), ("n16", 16, 32, 37), ("wave", 20, 33, 13), ("wave", 32, 64, 13),
           ("gram", 33, 40, 6), ("gram", 48, 96, 6)]
USED = {"n16": [0, 1] + list(range(3, 12)), "wave": list(range(12)), "gram": list(range(19))}
# x, lam and iters bitwise equal to qpb_solve's, as observed on an MI355X
# (status and active are asserted equal for every shape).  At n = 16, m = 32
# qpb_solve launches the FULL instantiation, the stamped build the padded one.
BITWISE_EQUAL_TO_PLAIN = {(16, 20), (16, 32), (20, 33), (32, 64), (33, 40), (48, 96)}


def _workgroups(build, B):
    """n16: four QPs per one-wave workgroup; wave: one QP per one-wave
    workgroup; gram: one workgroup per QP up to the CU count (B is below it),
    whose first wave alone stamps."""
    return (B + 3) // 4 if build == "n16" else B


def _sections_call(qpb, n, m, B, ins, outs, sections, sections_len, flags=0):
    d = qpb.Desc(n, m, B, 0, flags, 0.0)
    ptr = [qpb._ptr(t) if t is not None else None for t in list(ins) + list(outs)]
    return qpb.lib().qpb_solve_sections(ctypes.byref(d), *ptr, qpb._ptr(sections) if sections is not None else None,
                                        sections_len, qpb._stream_ptr(None))


def _new_outs(B, n, m):
    outs = [torch.empty((B, n), dtype=torch.float64, device="cuda"),
            torch.empty((B, m), dtype=torch.float64, device="cuda"),
            torch.empty((B, (m + 31) // 32), dtype=torch.int32, device="cuda"),
            torch.empty((B,), dtype=torch.int32, device="cuda"), torch.empty((B,), dtype=torch.int32, device="cuda")]
    for o in outs:
        o.view(torch.uint8).fill_(FILL)
    return outs


def _sections_buffer():
    buf = torch.zeros(SECTIONS_LEN + GUARD_WORDS, dtype=torch.int64, device="cuda")
    buf[SECTIONS_LEN:] = GUARD_VALUE
    return buf


def _shifted(n, m, B):
    import oracle as O
    return O.family_shifted(1000 + n + m, B, n, m)


@pytest.mark.parametrize("case", STAMPED, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in STAMPED])
def test_stamped_build(qpb, case):
    build, n, m, B = case
    H, f, A, b, xc = _shifted(n, m, B)
    ins = _dev(H, f, A, b)
    plain = _host(qpb.solve(*ins))
    outs, buf = _new_outs(B, n, m), _sections_buffer()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    rc = _sections_call(qpb, n, m, B, ins, outs, buf, SECTIONS_LEN)
    e1.record()
    assert rc == 0, (rc, qpb.lib().qpb_last_error())
    got = _host(outs)
    ticks_call = e0.elapsed_time(e1) * 1e5  # ms -> ticks of 100 MHz
    # the solve
    assert np.array_equal(got[3], plain[3]) and np.array_equal(got[2], plain[2])
    _check_parity(qpb, H, f, A, b, got, _oracle(("shifted", n, m, B), H, f, A, b, xc), f"stamped {build} {n}x{m}")
    equal = _same([got[0], got[1], got[4]], [plain[0], plain[1], plain[4]])
    print(f"stamped {build} {n}x{m}: x, lam, iters bitwise equal to the plain build: {equal}")
    assert equal == ((n, m) in BITWISE_EQUAL_TO_PLAIN)
    # the counters
    raw = buf.cpu().numpy()
    assert (raw[SECTIONS_LEN:] == GUARD_VALUE).all(), "guard words written"
    rows = raw[:SECTIONS_LEN].reshape(256, 20)
    wgs = _workgroups(build, B)
    assert (rows >= 0).all()
    assert (rows[wgs:] == 0).all(), np.nonzero(rows[wgs:])
    unused = [c for c in range(20) if c not in USED[build]]
    assert (rows[:, unused] == 0).all(), np.nonzero(rows[:, unused])
    total = int(rows.sum())
    print(f"stamped {build} {n}x{m}: {total} ticks over {wgs} waves, the call took {ticks_call:.0f} ticks; "
          f"per section {rows.sum(axis=0).tolist()}")
    assert total > 0
    if build != "gram":  # one QP or four per workgroup: each has stamped (gi_gram's walk a queue)
        assert (rows[:wgs].sum(axis=1) > 0).all()
    # no wave runs longer than the call: a wrapped or negative interval breaks this
    assert total <= wgs * ticks_call, (total, wgs, ticks_call)
    # the entry point adds into the buffer
    outs2 = _new_outs(B, n, m)
    assert _sections_call(qpb, n, m, B, ins, outs2, buf, SECTIONS_LEN) == 0
    assert _same(_host(outs2), got)
    raw2 = buf.cpu().numpy()
    assert (raw2[:SECTIONS_LEN] >= raw[:SECTIONS_LEN]).all() and raw2[:SECTIONS_LEN].sum() > total
    assert (raw2[SECTIONS_LEN:] == GUARD_VALUE).all()


def _unchanged(tensors, fill):
    torch.cuda.synchronize()
    return all(bool((t.view(torch.uint8) == fill).all()) for t in tensors)


def test_sections_argument_checks(qpb):
    n, m, B = 16, 32, 37
    H, f, A, b, _ = _shifted(n, m, B)
    ins = _dev(H, f, A, b)
    outs = _new_outs(B, n, m)
    buf = torch.full((SECTIONS_LEN + GUARD_WORDS,), 0, dtype=torch.int64, device="cuda")
    buf.view(torch.uint8).fill_(FILL)
    # a buffer one counter short: refused, nothing written
    assert _sections_call(qpb, n, m, B, ins, outs, buf, SECTIONS_LEN - 1) == qpb.ERR_INVALID_ARG
    assert _unchanged(outs + [buf], FILL)
    # no buffer, and the shapes without a stamped build
    assert _sections_call(qpb, n, m, B, ins, outs, None, SECTIONS_LEN) == qpb.ERR_UNSUPPORTED
    for n2, m2 in ((16, 16), (7, 14)):
        H2, f2, A2, b2, _ = _shifted(n2, m2, B)
        outs2 = _new_outs(B, n2, m2)
        assert _sections_call(qpb, n2, m2, B, _dev(H2, f2, A2, b2), outs2, buf,
                              SECTIONS_LEN) == qpb.ERR_UNSUPPORTED, (n2, m2)
        assert _unchanged(outs2, FILL)
    assert _unchanged(outs + [buf], FILL)
    # the array pointers are checked as qpb_solve checks them: H, x, status, and lam with m > 0
    for which in ("H", "x", "status", "lam"):
        i2, o2 = list(ins), list(outs)
        if which == "H":
            i2[0] = None
        else:
            o2[{"x": 0, "lam": 1, "status": 3}[which]] = None
        assert _sections_call(qpb, n, m, B, i2, o2, buf, SECTIONS_LEN) == qpb.ERR_INVALID_ARG, which
        assert _unchanged(outs + [buf], FILL), which
    # and the same pointers are accepted again
    buf.zero_()
    assert _sections_call(qpb, n, m, B, ins, outs, buf, SECTIONS_LEN) == 0
    assert _same(_host(outs), _host(qpb.solve(*ins)))


# ----------------------------------------------------------------------- b. flags
def _conditioned(seed, B, n, m):
    import oracle as O
    return _dev(*O.family_conditioned(seed, B, n, m=m, box=10.0, kind="dense"))


_INPUTS = {}


def _inputs(n, m, B):
    """Device inputs per shape, made once and shared (never modified)."""
    if (n, m, B) not in _INPUTS:
        _INPUTS[(n, m, B)] = _conditioned(6000 + n + m, B, n, m)
    return _INPUTS[(n, m, B)]


def _rows(sol, idx):
    return [a[idx] for a in sol]


@pytest.mark.parametrize("n,m,flag,period,B", [(16, 32, FLAG_DIAG_L2, 512, 1030), (7, 14, FLAG_DIAG_L2, 512, 1030),
                                               (16, 32, FLAG_DIAG_MALL, 16384, 16384 + 5)],
                         ids=["L2-16x32", "L2-7x14", "MALL-16x32"])
def test_diag_flags_alias_the_inputs(qpb, n, m, flag, period, B):
    """gi_dense_kernel with DIAG_L2 (DIAG_MALL): QP k reads the inputs of QP
    k mod 512 (16384) and writes its own outputs: they equal QP (k mod
    period)'s, which for k < period are a plain solve's."""
    ins = _inputs(n, m, B)
    plain = _host(qpb.solve(*ins))
    diag = _host(qpb.solve(*ins, flags=flag))
    k = np.arange(B)
    assert _same(_rows(diag, k[:period]), _rows(plain, k[:period]))
    assert _same(_rows(diag, k), _rows(diag, k % period))
    # validity: without the flag the QPs past the period do differ from their aliases
    assert not np.array_equal(plain[0][period:], plain[0][:B - period])


IGNORED_ROUTES = [("gi_dense", 16, 32, 37, 0), ("gi_wave", 20, 33, 13, 0), ("gi_gram", 48, 96, 6, 0)]


@pytest.mark.parametrize("route", IGNORED_ROUTES, ids=[r[0] for r in IGNORED_ROUTES])
def test_retired_flags_are_ignored(qpb, route):
    """Flag values 4, 8 and 128: accepted and ignored (qpb.h)."""
    name, n, m, B, base = route
    ins = _inputs(n, m, B)
    plain = _host(qpb.solve(*ins, flags=base))
    for fl in RETIRED:
        assert _same(_host(qpb.solve(*ins, flags=base | fl)), plain), fl


L2_ELSEWHERE = [("gi_wave-20x33", 20, 33, 520, 0), ("gi_gram-48x96", 48, 96, 520, 0),
                ("gi_wave-diag-7x14", 7, 14, 520, FLAG_DIAG_WAVE)]


@pytest.mark.parametrize("route", L2_ELSEWHERE, ids=[r[0] for r in L2_ELSEWHERE])
def test_diag_l2_is_ignored_outside_its_class(qpb, route):
    """QPB_FLAG_DIAG_L2 belongs to the n <= 16, m <= 32 kernel: the wavefront
    and Gram classes, and n <= 16 under DIAG_WAVE, ignore it (batches past
    512 QPs, so aliasing would show)."""
    name, n, m, B, base = route
    ins = _inputs(n, m, B)
    plain = _host(qpb.solve(*ins, flags=base))
    assert not np.array_equal(plain[0][512:], plain[0][:B - 512])
    assert _same(_host(qpb.solve(*ins, flags=base | FLAG_DIAG_L2)), plain)


def test_solve_box_flags_select_nothing(qpb):
    """qpb_solve_box at n = 7 with every flag bit set (past 512 QPs): equal to flags = 0."""
    import oracle as O
    n, B = 7, 520
    H, f, _, _ = O.family_conditioned(6100, B, n, box=10.0)
    ins = _dev(H, f, np.full((B, n), -10.0), np.full((B, n), 10.0))
    plain = _host(qpb.solve_box(*ins))
    outs = _new_outs(B, n, 2 * n)
    d = qpb.Desc(n, 2 * n, B, 0, 1 | 4 | 8 | 16 | 32 | 64 | 128 | 256, 0.0)
    rc = qpb.lib().qpb_solve_box(ctypes.byref(d), *[qpb._ptr(t) for t in ins + outs], qpb._stream_ptr(None))
    assert rc == 0, (rc, qpb.lib().qpb_last_error())
    assert _same(_host(outs), plain)
    assert not np.array_equal(plain[0][512:], plain[0][:B - 512])


# --------------------------------------------------------------------- c. qf_eval
QF_B = 257  # a ragged last block of the 256-thread launch
QF_R = -3.5
U = 2.0 ** -53


@pytest.mark.parametrize("n", [1, 7, 16, 128, 300])
def test_qf_eval(qpb, n):
    """1/2 x'Px + q'x + r against numpy.longdouble.  The kernel is built
    without contraction, so every operation rounds once, and a term
    P_ik x_k x_i passes through at most 2n + 2 of them (its product, n - 1
    additions of the row sum, the product with x_i, n - 1 additions over the
    rows, + q'x, + r; the halving is exact), the terms of q'x and r through
    fewer.  With gamma_k = k u / (1 - k u) and gamma_{2n+2} <= 2 (n + 2) u for
    every n here,
        |out - ref| <= 2 (n + 2) 2^-53 (1/2 |x|'|P||x| + |q|'|x| + |r|).
    The reference's own error (64-bit significand) is 2^-11 of that."""
    rs = np.random.default_rng(6200 + n)
    P = rs.uniform(-1e3, 1e3, (QF_B, n, n))
    q = rs.uniform(-1e3, 1e3, (QF_B, n))
    x = rs.uniform(-1e3, 1e3, (QF_B, n))
    Pd, qd, xd = _dev(P, q, x)
    out = qpb.qf_eval(Pd, qd, QF_R, xd)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    L = np.longdouble
    assert np.finfo(L).nmant >= 63
    ref = np.empty(QF_B, dtype=L)
    mag = np.empty(QF_B)
    for k in range(QF_B):
        Pk, qk, xk = P[k].astype(L), q[k].astype(L), x[k].astype(L)
        ref[k] = L(0.5) * (xk @ (Pk @ xk)) + qk @ xk + L(QF_R)
        mag[k] = float(L(0.5) * (np.abs(xk) @ (np.abs(Pk) @ np.abs(xk))) + np.abs(qk) @ np.abs(xk) + abs(QF_R))
    err = np.abs(out.astype(L) - ref).astype(np.float64)
    bound = 2.0 * (n + 2) * U * mag
    print(f"qf_eval n={n}: largest error / bound = {(err / bound).max():.3e}")
    assert np.isfinite(out).all()
    assert (err <= bound).all(), (n, (err / bound).max())


def test_qf_eval_edges(qpb):
    n = 16
    P, q, x = _dev(np.ones((1, n, n)), np.ones((1, n)), np.ones((1, n)))
    out = torch.empty((1,), dtype=torch.float64, device="cuda")
    out.view(torch.uint8).fill_(FILL)
    call = lambda B, o: qpb.lib().qpb_qf_eval(n, B, qpb._ptr(P), qpb._ptr(q), QF_R, qpb._ptr(x), o,  # noqa: E731
                                               qpb._stream_ptr(None))
    assert call(0, qpb._ptr(out)) == 0  # an empty batch: success, nothing written
    assert _unchanged([out], FILL)
    assert call(1, None) == qpb.ERR_INVALID_ARG
    assert _unchanged([out], FILL)
    assert call(1, qpb._ptr(out)) == 0
    torch.cuda.synchronize()
    assert float(out[0]) == 0.5 * n * n + n + QF_R
