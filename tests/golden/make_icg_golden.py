"""Records tests/golden/icg_parent.npz: u, its iteration count and one S-apply of every case of tests/icg_cases.py, as the
build in the tree computes them on an MI355X, and the SHA-256 of every case's inputs. Run ONCE, on the commit BEFORE a change to the
interior CG's kernels or to how its `Pl` is selected; tests/test_gpu_icg_bits.py then holds the changed build to these bits.

    python tests/golden/make_icg_golden.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as graft  # noqa: E402
import icg_cases as cases  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "icg_parent.npz")
    pkg = graft.load_package()
    results = cases.run_all(pkg.api, pkg.api.Context(0))
    assert sorted(results) == sorted(cases.NAMES)
    for name, (u, it, y) in results.items():
        print(f"{name}: n = {u.size} it = {it} max|u| = {np.abs(u).max() if u.size else 0.0:.6e}")
    np.savez_compressed(out, **cases.pack(results, cases.input_digests(pkg.fem)))
    print("wrote", out, os.path.getsize(out), "bytes")
