"""The n <= 16 kernel addresses memory from one scalar base per group of four
QPs (a wavefront) plus a 32-bit offset per lane, and bounds its unrolled loops
by scalar maxima over the four active-set sizes.  On the cases of
tests/addr_cases.py (its docstring says why each is there):

  1. all five outputs are bitwise those of the gi_dense v11.6 library, the
     revision before the scalar bases (tests/golden/gi_dense_v116_addr.npz,
     recorded by tools/record_addr_golden.py; gi_dense_v116_addr.json says how);
  2. x is within 1e-9 of the planted solution (the data are small integers, the
     solution exact: tests/planted.py);
  3. the `active` case really ends with 0, 1, 8, 9 and 16 active rows, mixed
     within its waves;
  4. with QPB_FLAG_DIAG_L2 and a batch above 512, QP g gets the outputs of QP
     g mod 512 solved directly.
"""
import json
import os

import numpy as np
import pytest

import addr_cases
from conftest import GOLDEN

X_ABS = 1e-9
FIELDS = ("x", "lam", "active", "status", "iters")
NAMES = ["b1", "b2", "b3", "b5", "b67", "offset", "16x16", "16x20", "12x32", "5x7", "16x0", "5x0", "eq", "active"]


@pytest.fixture(scope="module")
def qpb():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import qpb as q
    return q


@pytest.fixture(scope="module")
def cases():
    return addr_cases.cases()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "gi_dense_v116_addr.npz"))


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(
        np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def test_the_cases_are_the_recorded_ones(cases):
    """The goldens belong to these inputs bit for bit (a changed generator shows here, not as a
    kernel regression), and every case is present."""
    meta = json.load(open(os.path.join(GOLDEN, "gi_dense_v116_addr.json")))
    assert list(cases) == NAMES == list(meta["cases"])
    assert addr_cases.input_digest(cases) == meta["inputs_sha256"]
    assert max(len(c.f) for c in cases.values()) <= 67


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_outputs_are_v116s_and_x_is_the_planted_one(qpb, cases, golden, name):
    c = cases[name]
    got = addr_cases.solve_case(qpb, c, offset=name == "offset")
    assert (got["status"] == qpb.OK).all(), got["status"]
    err = float(np.abs(got["x"] - c.x).max())
    print(name, "max |x - x*|", err, "iters mean", got["iters"].mean())
    for k in FIELDS:
        want = golden[f"{name}_{k}"]
        assert _same_bits(got[k], want), (name, k, int((got[k] != want).sum()))
    assert err <= X_ABS, (name, err)


@pytest.mark.gpu
def test_active_case_mixes_0_1_8_9_16_active_rows(qpb, cases):
    got = addr_cases.solve_case(qpb, cases["active"])
    nact = qpb.active_mask_to_bool(got["active"], 32).sum(axis=1)
    assert nact.reshape(-1, 4).tolist() == [list(w) for w in addr_cases.ACTIVE_WAVES]


@pytest.mark.gpu
def test_diag_l2_reads_qp_g_mod_512(qpb):
    """579 = 512 + 67 QPs (a ragged last group): with the flag, QP g reads the inputs of QP
    g mod 512 -- its outputs are those of that QP solved without the flag, bitwise."""
    import torch
    B = 579
    H, f, A, b = qpb.generate(16, B, 20261019, family="dense", shift=1.0, box=10.0, device=torch.device("cuda", 0))
    direct = qpb.solve(H[:512].contiguous(), f[:512].contiguous(), A[:512].contiguous(), b[:512].contiguous())
    flagged = qpb.solve(H, f, A, b, flags=qpb.FLAG_DIAG_L2)
    torch.cuda.synchronize()
    src = np.arange(B) % 512
    assert len(np.unique(direct.iters.cpu().numpy())) > 2  # QPs that differ from one another
    for k in FIELDS:
        want = getattr(direct, k).cpu().numpy()[src]
        got = getattr(flagged, k).cpu().numpy()
        assert _same_bits(got, want), (k, int((got != want).sum()))
