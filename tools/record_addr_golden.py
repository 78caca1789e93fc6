#!/usr/bin/env python3
"""Record the built library's outputs on the cases of tests/addr_cases.py, as
the bitwise fixture of tests/test_gpu_dense_addressing.py:
  python tools/record_addr_golden.py OUTDIR [TAG]
-> OUTDIR/gi_dense_<TAG>_addr.npz (TAG default v116): <case>_{x,lam,active,
status,iters} for every case, and OUTDIR/gi_dense_<TAG>_addr.json, its
provenance (library revision, shapes, the digest of the inputs, sha256).
Run it with the library the fixture is to pin (QPB_LIB names another build).
The inputs are not stored: tests/planted.py rebuilds them from their seeds."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "embedded-qp-solver_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import addr_cases  # noqa: E402
import qpb  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1]
    tag = sys.argv[2] if len(sys.argv) > 2 else "v116"
    os.makedirs(out, exist_ok=True)
    cs = addr_cases.cases()
    arrs, shapes = {}, {}
    for name, c in cs.items():
        got = addr_cases.solve_case(qpb, c, offset=name == "offset")
        for k, v in got.items():
            arrs[f"{name}_{k}"] = v
        m = 0 if c.A is None else c.A.shape[1]
        shapes[name] = {"batch": len(c.f), "n": c.f.shape[1], "m": m, "meq": c.meq}
        print(name, shapes[name], "status", np.bincount(got["status"]).tolist(), "iters mean", got["iters"].mean(),
              "max |x - x*|", float(np.abs(got["x"] - c.x).max()))
    npz = f"gi_dense_{tag}_addr.npz"
    np.savez_compressed(os.path.join(out, npz), **arrs)
    meta = {"file": npz, "cases": shapes, "inputs": "tests/addr_cases.py cases(), rebuilt from seeds by tests/planted.py",
            "inputs_sha256": addr_cases.input_digest(cs), "library": qpb.version().split(":")[0] + ")",
            "made_by": "tools/record_addr_golden.py on an MI355X with the library named above: the five outputs of "
                       "qpb_solve (qpb_solve_eq for the case eq) per case; the case offset through views 3 QPs into "
                       "larger allocations",
            "sha256": hashlib.sha256(open(os.path.join(out, npz), "rb").read()).hexdigest()}
    open(os.path.join(out, f"gi_dense_{tag}_addr.json"), "w").write(json.dumps(meta, indent=1) + "\n")
