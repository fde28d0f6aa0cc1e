"""Records tests/golden/full_split_parent.npz: every result of tests/full_split_cases.py as the build in the tree computes it
on an MI355X, with the inputs and their digests. Run ONCE, on the commit BEFORE the LORASC and the Neumann-Neumann induced
operator were given one shared interior/Γ split; tests/test_gpu_full_split.py then holds the changed build to these bits.

    python tests/golden/make_full_split_golden.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as graft  # noqa: E402
import full_split_cases as cases  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "full_split_parent.npz")
    pkg = graft.load_package()
    doc = cases.inputs(pkg.fem)
    doc.update(cases.run_all(pkg.api, pkg.fem, pkg.api.Context(0)))
    for k, v in doc.items():
        if k.startswith("solve/") and k.endswith("/it"):
            print(f"{k} = {int(v)}, res_norm[-1] = {doc[k[:-2] + 'res_norm'][-1]:.3e}")
        elif not k.startswith(("in/", "sha/", "solve/")):
            print(f"{k}: n = {v.size}, |z| = {np.linalg.norm(v):.6e}")
    np.savez_compressed(out, **doc)
    print("wrote", out, os.path.getsize(out), "bytes")
