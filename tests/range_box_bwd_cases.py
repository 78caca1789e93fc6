"""TEST INFRASTRUCTURE ONLY: the batches of tests/test_gpu_range_box_backward.py
(numpy, no GPU), so that tests/test_range_box_bwd_cases.py can hold the very
inputs the GPU tests differentiate to the numpy oracle.

`inputs` is tests/range_box_oracle.py's family, with H[0] for the batch where H
is shared and, where G is shared, G[0] with bounds regenerated around G0 xc (xc
stays strictly feasible) at the family's own width.
"""
import numpy as np

import range_box_oracle as BO

COUNT = 24
RAGGED = [(16, 16, 2), (12, 20, 0)]
RAGGED_COUNTS = [1, 3, 5, 65]
SHARED_SHAPES = [(16, 16, 2), (12, 20, 0), (20, 9, 0), (32, 32, 3)]
SHARED_COUNTS = [24, 261]
SHARED_FORMS = [(True, False), (False, True), (True, True)]  # H shared, G shared


def inputs(count, n, mg, meq, share_h=False, share_g=False):
    """(H, f, G, bl, bu, lb, ub, xc, rng): H (n, n) where shared, G (mg, n) where
    shared; rng is the generator the GPU tests draw their cotangents from next."""
    H, f, G, bl, bu, lb, ub, xc = BO.box_family(count, n, mg, meq)
    rng = np.random.default_rng([31, n, mg, count])
    if share_h:
        H = H[0]
    if share_g and mg:
        G = G[0]
        gxc = np.einsum("ij,bj->bi", G, xc)
        # (the family's own width, U(0.1, 1) 10: with rows ten times tighter no variable's bound binds
        # at (12, 20), tests/test_range_box_bwd_cases.py)
        bu = gxc + rng.uniform(0.1, 1.0, size=gxc.shape) * 10.0
        bl = gxc - rng.uniform(0.1, 1.0, size=gxc.shape) * 10.0
        bl[:, :meq] = bu[:, :meq] = gxc[:, :meq]
    return H, f, G, bl, bu, lb, ub, xc, rng
