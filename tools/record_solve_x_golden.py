#!/usr/bin/env python3
"""Record tests/golden/gi_dense_v118_solve_x.npz: the outputs of the two other
users of row16::solve_x, qpb_solve_box and qpb_solve_box_backward at n = 16, on
a batch of 64 box QPs, from the library that is built -- run it on the commit
BEFORE a change to solve_x; tests/test_gpu_dense_output_phase.py then holds
the changed library to these bits.

  python tools/record_solve_x_golden.py [output.npz]

The inputs are stored beside the outputs, so the test does not depend on a
generator's stream: a well-conditioned random H, f scaled so that about a third
of the variables end on a bound, and a smooth cotangent gx for the backward.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "embedded-qp-solver_amd"))
import torch  # noqa: E402

import qpb  # noqa: E402

N, B = 16, 64


def inputs():
    rs = np.random.default_rng(118)
    M = rs.standard_normal((B, N, N))
    H = np.eye(N)[None] + np.einsum("bij,bik->bjk", M, M) / N
    f = 3.0 * rs.standard_normal((B, N))
    lb = -0.5 - rs.random((B, N))
    ub = 0.5 + rs.random((B, N))
    gx = rs.standard_normal((B, N))
    return H, f, lb, ub, gx


def main(path):
    dev = torch.device("cuda", 0)
    H, f, lb, ub, gx = inputs()
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (H, f, lb, ub, gx)]
    sol = qpb.solve_box(t[0], t[1], t[2], t[3])
    gH, gf, glb, gub = qpb.solve_box_backward(t[0], sol, t[4])
    torch.cuda.synchronize()
    out = {"H": H, "f": f, "lb": lb, "ub": ub, "gx": gx}
    out.update({k: getattr(sol, k).cpu().numpy() for k in ("x", "lam", "active", "status", "iters")})
    out.update({"gH": gH.cpu().numpy(), "gf": gf.cpu().numpy(), "glb": glb.cpu().numpy(), "gub": gub.cpu().numpy()})
    nact = qpb.active_mask_to_bool(out["active"], 2 * N).sum(axis=1)
    assert (out["status"] == 0).all(), out["status"]
    np.savez_compressed(path, library=np.array(qpb.version()), **out)
    print(f"{path}: {os.path.getsize(path)} bytes, active bounds per QP {nact.min()}..{nact.max()}, "
          f"iters {out['iters'].min()}..{out['iters'].max()}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "gi_dense_v118_solve_x.npz"))
