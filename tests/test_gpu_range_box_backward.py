"""qpb_solve_range_box_backward on the GPU against its specification: every
output equals, bit for bit (np.array_equal on int64 views), what
qpb_solve_backward_dual writes on the materialised A' = [G; I] built here, its
gA' cut to the rows of G and its gb' routed by the `lower` bits
(tests/range_box_bwd_harness.py).  The native call never sees A'.

Inputs are tests/range_box_oracle.py's family; the forward is
qpb.solve_range_box on the GPU, the cotangents are seeded normals.  The shapes
are that file's, one per code path: the N16 and padded dense loads at one and
two rows per lane, unit rows straddling the two row registers, mg = 0 without a
G pointer, the class edge (16, 17) and the wave forms up to two mask words.
Every output lives in a NaN-filled arena with guards: nothing outside a wanted
output is written, and the place of a NULL output stays untouched.

One check is independent of the materialised kernels: the outputs solve the KKT
system of the materialised problem (a dense numpy solve, tests/dual_oracle.py)
to the project's X_TOL = 1e-6 and KKT_TOL = 1e-9.
"""
import numpy as np
import pytest

import dual_oracle as DO
import range_box_bwd_cases as BC
import range_box_bwd_harness as BH
import range_box_oracle as BO
import range_oracle as RO
from bwd_harness import KKT_TOL, X_TOL, rel as _rel

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

COUNT = BC.COUNT
NAMES = BH.NAMES
RAGGED = BC.RAGGED
SHARED_SHAPES = BC.SHARED_SHAPES
MASK_SHAPES = [(16, 16, 0), (20, 9, 0)]
KKT_SHAPES = [(16, 16, 2), (12, 20, 0), (20, 9, 0)]


@pytest.fixture(scope="module")
def qpb():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


_SOLVED = {}


def _case(qpb, count, n, mg, meq, share_h=False, share_g=False):
    """A solved batch on the device, made once and shared (never modified):
    H, G (None at mg == 0), x, lam, act, low, st, gx, gl."""
    key = (count, n, mg, meq, share_h, share_g)
    if key not in _SOLVED:
        # (tests/test_range_box_bwd_cases.py holds these very inputs to the numpy oracle)
        H, f, G, bl, bu, lb, ub, xc, rng = BC.inputs(count, n, mg, meq, share_h, share_g)
        Hd, Gd = BH.dev(H), (BH.dev(G) if mg else None)
        sol = qpb.solve_range_box(Hd, BH.dev(f), Gd, BH.dev(bl) if mg else None, BH.dev(bu) if mg else None,
                                  BH.dev(lb), BH.dev(ub), meq)
        torch.cuda.synchronize()
        assert (sol.status == qpb.OK).all()
        _SOLVED[key] = dict(H=Hd, G=Gd, x=sol.x, lam=sol.lam, act=sol.active, low=sol.lower, st=sol.status,
                            gx=BH.dev(rng.standard_normal((count, n))),
                            gl=BH.dev(rng.standard_normal((count, mg + n))))
    return _SOLVED[key]


def _args(c):
    return c["H"], c["G"], c["x"], c["lam"], c["act"], c["low"], c["st"], c["gx"]


# ------------------------------------------------------------ 1. every output, every subset
@pytest.mark.parametrize("n,mg,meq", BO.SHAPES)
def test_outputs_are_the_materialised_calls(qpb, n, mg, meq):
    c = _case(qpb, COUNT, n, mg, meq)
    for gl in (None, c["gl"]):
        ref = BH.materialised(qpb, *_args(c), gl)
        out = BH.native(qpb, *_args(c), gl)
        assert set(out) == {k for k in NAMES if ref[k].size}
        BH.same(out, ref)
        assert np.array_equal(out["H"], out["H"].transpose(0, 2, 1))
        # every subset of one output, and all but one
        for k in NAMES:
            if ref[k].size:
                BH.same(BH.native(qpb, *_args(c), gl, need=(k,)), ref)
            rest = tuple(j for j in NAMES if j != k)
            if any(ref[j].size for j in rest):
                BH.same(BH.native(qpb, *_args(c), gl, need=rest), ref)
    # the cotangent on lam is not a no-op, and the solve has bounds on both sides to route
    assert not np.array_equal(BH.native(qpb, *_args(c), None, need=("f",))["f"], out["f"])
    assert (out["lb"] != 0).any() and (out["ub"] != 0).any()


@pytest.mark.parametrize("n,mg,meq", RAGGED)
@pytest.mark.parametrize("count", BC.RAGGED_COUNTS)
def test_ragged_last_wavefront(qpb, count, n, mg, meq):
    c = _case(qpb, count, n, mg, meq)
    for gl in (None, c["gl"]):
        BH.same(BH.native(qpb, *_args(c), gl), BH.materialised(qpb, *_args(c), gl))


def test_python_binding_returns_the_same_bits(qpb):
    n, mg, meq = 16, 16, 2
    c = _case(qpb, COUNT, n, mg, meq)
    sol = qpb.RangeSolution(c["x"], c["lam"], c["act"], c["low"], c["st"], None)
    for gl in (None, c["gl"]):
        ref = BH.materialised(qpb, *_args(c), gl)
        got = qpb.solve_range_box_backward(c["H"], c["G"], sol, c["gx"], gl)
        torch.cuda.synchronize()
        BH.same({k: t.cpu().numpy() for k, t in zip(NAMES, got)}, ref)
        got = qpb.solve_range_box_backward(c["H"], c["G"], sol, c["gx"], gl, need=("G", "ub"))
        assert [t is None for t in got] == [True, True, False, True, True, True, False]
        host = qpb.solve_range_box_backward_host(c["H"].cpu().numpy(), c["G"].cpu().numpy(),
                                                 qpb.RangeSolution(*(None if t is None else t.cpu().numpy() for t in sol)),
                                                 c["gx"].cpu().numpy(), None if gl is None else gl.cpu().numpy())
        BH.same(dict(zip(NAMES, host)), ref)
    # G = None: no gradient for it, the variables' bounds alone
    c0 = _case(qpb, COUNT, 16, 0, 0)
    sol0 = qpb.RangeSolution(c0["x"], c0["lam"], c0["act"], c0["low"], c0["st"], None)
    got = qpb.solve_range_box_backward(c0["H"], None, sol0, c0["gx"])
    assert got[2] is None and tuple(got[3].shape) == (COUNT, 0) and tuple(got[5].shape) == (COUNT, 16)


# ------------------------------------------------------------ 2. shared operands: the summed gradients
@pytest.mark.parametrize("n,mg,meq", SHARED_SHAPES)
@pytest.mark.parametrize("count", BC.SHARED_COUNTS)
@pytest.mark.parametrize("share_h,share_g", BC.SHARED_FORMS)
def test_shared_operands_sum_to_the_same_bits(qpb, count, n, mg, meq, share_h, share_g):
    c = _case(qpb, count, n, mg, meq, share_h, share_g)
    assert c["H"].dim() == (2 if share_h else 3) and c["G"].dim() == (2 if share_g else 3)
    for gl in (None, c["gl"]):
        ref = BH.materialised(qpb, *_args(c), gl)
        assert ref["H"].shape == tuple(c["H"].shape) and ref["G"].shape == tuple(c["G"].shape)
        out = BH.native(qpb, *_args(c), gl)
        BH.same(out, ref)
        if share_h:
            assert np.array_equal(out["H"], out["H"].T)
        # the workspace paths: gf NULL (dx in the workspace), and the bound arrays NULL with gG wanted
        BH.same(BH.native(qpb, *_args(c), gl, need=("H", "G")), ref)
        BH.same(BH.native(qpb, *_args(c), gl, need=("G",)), ref)
        BH.same(BH.native(qpb, *_args(c), gl, need=("H", "bl", "ub")), ref)
    # a second call on another stream: the same bits
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    BH.same(BH.native(qpb, *_args(c), c["gl"], stream=s), ref)


# ------------------------------------------------------------ 3. hand-made masks
def _hand_made(n, mg):
    """(G, x, lam, act, low, labels): one QP per case, three seeded copies each."""
    m = mg + n
    rng = np.random.default_rng([37, n, mg])
    cases = []

    def add(label, act, low, lam=None, G=None):
        for _ in range(3):
            g = rng.standard_normal((mg, n)) if G is None else G(rng.standard_normal((mg, n)))
            lm = rng.standard_normal(m) + np.sign(rng.standard_normal(m))
            cases.append((label, g, rng.standard_normal(n), lm if lam is None else lam(lm), act.copy(), low.copy()))

    rows, vars_ = np.arange(m) < mg, np.arange(m) >= mg
    half = rng.random(m) < 0.5
    add("variables only, |W| = n", vars_, vars_ & half)
    rows_only = rows & (np.arange(m) < n)
    add("rows only", rows_only, rows_only & half)
    add("more than n bits: all set", np.ones(m, bool), half)
    some = np.zeros(m, bool)
    some[[0, 2, mg + 1, mg + 3, m - 1]] = True
    add("lower bits on inactive rows", some, ~some | half)
    for sign in (1.0, -1.0):
        j = 3

        def unit_row(g, sign=sign, j=j):
            g[2] = 0.0
            g[2, j] = sign
            return g

        dep = some.copy()
        dep[[2, mg + j]] = True  # the row and the variable it repeats: the skip lands on the variable
        add(f"G row {sign:+.0f} e_j beside variable j", dep, dep & half, G=unit_row)

    def weak(lm):
        lm[mg + 1] = 0.0
        return lm

    add("a weakly active variable", some, some & half, lam=weak)
    labels = [c[0] for c in cases]
    G, x, lam, act, low = (np.array([c[k] for c in cases]) for k in range(1, 6))
    return G, x, lam, act, low, labels


@pytest.mark.parametrize("n,mg,meq", MASK_SHAPES)
def test_hand_made_masks(qpb, n, mg, meq):
    m = mg + n
    G, x, lam, act, low, labels = _hand_made(n, mg)
    Bq = len(labels)
    H = BO.box_family(Bq, n, mg, meq)[0]
    aw, lw = RO.pack_bits(act), RO.pack_bits(low)
    if m % 32:
        # bits >= m' of the last word are ignored, in both masks
        aw[1::2, -1] |= np.uint32((0xFFFFFFFF << (m % 32)) & 0xFFFFFFFF)
        lw[::3, -1] |= np.uint32((0xFFFFFFFF << (m % 32)) & 0xFFFFFFFF)
    rng = np.random.default_rng([38, n, mg])
    args = (BH.dev(H), BH.dev(G), BH.dev(x), BH.dev(lam), BH.dev(aw.view(np.int32)), BH.dev(lw.view(np.int32)),
            None, BH.dev(rng.standard_normal((Bq, n))))
    for gl in (None, BH.dev(rng.standard_normal((Bq, m)))):
        ref = BH.materialised(qpb, *args, gl)
        out = BH.native(qpb, *args, gl)
        BH.same(out, ref)
        gb = np.concatenate([out["bl"] + out["bu"], out["lb"] + out["ub"]], axis=1)
        for i, label in enumerate(labels):
            # a row outside W gets zeros, whatever its lower bit says
            assert (gb[i][~act[i]] == 0.0).all() and (out["G"][i][~act[i, :mg]] == 0.0).all(), label
            if "beside variable j" in label:
                assert gb[i][2] != 0.0 and gb[i][mg + 3] == 0.0, label  # the later of the two is the skipped one
            if label.startswith("more than n bits"):
                assert np.count_nonzero(gb[i]) <= n, label
    # lower NULL: every routed element goes to the upper arrays
    noL = args[:5] + (None,) + args[6:]
    out = BH.native(qpb, *noL, None, need=("H", "f", "G", "bu", "ub"))
    BH.same(out, BH.materialised(qpb, *noL, None))


# ------------------------------------------------------------ 4. poison
@pytest.mark.parametrize("n,mg,meq", [(16, 16, 2), (20, 9, 0)])
def test_poison_outside_the_active_set_and_failed_qps(qpb, n, mg, meq):
    """lam and glam outside W are ignored, NaN included: the outputs with NaN
    there are finite and equal, bit for bit, those with 0.0 in its place (as
    tests/test_gpu_backward_dual.py asserts it of the materialised call), with
    and without a status array.  NaN in x, lam and glam of QPs whose status is
    not OK: zeros in every per-QP output, exactly 0 in the sums.  (The poisoned
    arrays are made on the host: a device-side where() takes its memory layout
    from the mask, and the C ABI reads row-major memory.)"""
    m = mg + n
    c = _case(qpb, COUNT, n, mg, meq)
    lam0, gl0, x0, st0 = (c[k].cpu().numpy() for k in ("lam", "gl", "x", "st"))
    inW = RO.unpack_bits(c["act"].cpu().numpy(), m)
    assert not (lam0[~inW] != 0).any()
    clean = BH.native(qpb, *_args(c), BH.dev(np.where(inW, gl0, 0.0)))
    BH.same(clean, BH.materialised(qpb, *_args(c), c["gl"]))  # (random values there are ignored as well)
    lam, gl = BH.dev(np.where(inW, lam0, np.nan)), BH.dev(np.where(inW, gl0, np.nan))
    assert bool(torch.isnan(lam).any()) and bool(torch.isnan(gl).any())
    for st in (c["st"], None):
        out = BH.native(qpb, c["H"], c["G"], c["x"], lam, c["act"], c["low"], st, c["gx"], gl)
        BH.same(out, clean)
        assert all(np.isfinite(v).all() for v in out.values())
        BH.same(out, BH.materialised(qpb, c["H"], c["G"], c["x"], lam, c["act"], c["low"], st, c["gx"], gl))
    # QPs whose status is not OK: NaN in their x, lam and glam, zeros in every per-QP output
    bad = np.zeros(COUNT, bool)
    bad[[1, 4, 5, COUNT - 1]] = True
    ignored = ~inW | bad[:, None]
    st = BH.dev(np.where(bad, 3, st0).astype(np.int32))
    spoil = lambda a, v: BH.dev(np.where(bad[:, None], v, a))  # noqa: E731
    x, lam, gl = spoil(x0, np.nan), BH.dev(np.where(ignored, np.nan, lam0)), BH.dev(np.where(ignored, np.nan, gl0))
    gx = c["gx"]
    out = BH.native(qpb, c["H"], c["G"], x, lam, c["act"], c["low"], st, gx, gl)
    BH.same(out, BH.materialised(qpb, c["H"], c["G"], x, lam, c["act"], c["low"], st, gx, gl))
    for k in NAMES:
        assert np.isfinite(out[k]).all(), k
        assert (out[k][bad].view(np.int64) == 0).all(), k  # +0.0, every element
        assert np.array_equal(out[k][~bad].view(np.int64), clean[k][~bad].view(np.int64)), k
    # ... and exactly 0 in the sums of a shared H and G: finite, the materialised call's bits, and
    # the same bits whatever those QPs hold (other, finite, values in the three arrays)
    Hs, Gs = c["H"][0].contiguous(), c["G"][0].contiguous()
    out = BH.native(qpb, Hs, Gs, x, lam, c["act"], c["low"], st, gx, gl)
    BH.same(out, BH.materialised(qpb, Hs, Gs, x, lam, c["act"], c["low"], st, gx, gl))
    assert all(np.isfinite(v).all() for v in out.values())
    again = BH.native(qpb, Hs, Gs, spoil(x0, 7.25), spoil(lam0, 7.25), c["act"], c["low"], st, gx, spoil(gl0, 7.25))
    BH.same(again, out, names=("H", "G"))


# ------------------------------------------------------------ 5. the KKT system itself
@pytest.mark.parametrize("n,mg,meq", KKT_SHAPES)
def test_outputs_solve_the_materialised_kkt_system(qpb, n, mg, meq):
    m = mg + n
    c = _case(qpb, COUNT, n, mg, meq)
    out = BH.native(qpb, *_args(c), c["gl"])
    H, G, x, lam, gx, gl = (c[k].cpu().numpy() for k in ("H", "G", "x", "lam", "gx", "gl"))
    act = RO.unpack_bits(c["act"].cpu().numpy(), m)
    low = RO.unpack_bits(c["low"].cpu().numpy(), m)
    A = np.concatenate([G, np.broadcast_to(np.eye(n), (COUNT, n, n))], axis=1)
    gb = np.concatenate([out["bl"] + out["bu"], out["lb"] + out["ub"]], axis=1)
    worst = dict.fromkeys(("H", "f", "G", "b"), 0.0)
    cert = np.zeros((COUNT, 2))
    for i in range(COUNT):
        gH, gf, gA, gbr = DO.backward(H[i], x[i], lam[i], A[i], act[i], gx[i], gl[i])
        for k, got, want in (("H", out["H"][i], gH), ("f", out["f"][i], gf), ("G", out["G"][i], gA[:mg]),
                             ("b", gb[i], gbr)):
            worst[k] = max(worst[k], float(_rel(got[None], want[None])[0]))
        cert[i] = DO.certificate(H[i], A[i], act[i], gx[i], gl[i], out["f"][i], gb[i])
    print(f"({n},{mg},{meq}): errors {worst} certificate stat {cert[:, 0].max():.2e} prim {cert[:, 1].max():.2e}")
    assert all(v <= X_TOL for v in worst.values()), worst
    assert cert.max() <= KKT_TOL, cert.max(axis=0)
    # the routing: an element sits in the lower array exactly where the row's lower bit is set
    glo = np.concatenate([out["bl"], out["lb"]], axis=1)
    ghi = np.concatenate([out["bu"], out["ub"]], axis=1)
    assert (glo[~low] == 0.0).all() and (ghi[low] == 0.0).all() and (gb[~act] == 0.0).all()
    assert (glo != 0).any() and (ghi != 0).any()
