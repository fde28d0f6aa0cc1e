"""Records tests/golden/krylov_parent.npz: x, `it` and the whole res_norm history (and the vectors the eigCG family returns) of
every case of tests/krylov_bits_cases.py, as the build in the tree computes them on an MI355X, and the SHA-256 of every
case's inputs. Run ONCE, on the commit BEFORE a change to the Krylov loop's kernels (csrc/kernels.hpp) or to how its form
is selected (csrc/solvers.hpp); tests/test_gpu_krylov_bits.py then holds the changed build to these bits.

    python tests/golden/make_krylov_golden.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as graft  # noqa: E402
import krylov_bits_cases as cases  # noqa: E402
from oracle import oracle as orc  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "krylov_parent.npz")
    pkg = graft.load_package()
    orc.build()
    ctx = pkg.api.Context(0)
    probs, eprobs = cases.probs_of(pkg.api, ctx, orc)
    digests = cases.input_digests(probs, eprobs)
    results = cases.run_all(pkg.api, ctx, probs, eprobs)
    assert sorted(results) == sorted(cases.NAMES)
    for name, r in results.items():
        print(f"{name}: n = {r[0].size} it = {r[1]} res_norm[end] = {r[2][-1] if len(r[2]) else 0.0:.6e}")
    np.savez_compressed(out, **cases.pack(results, digests))
    print("wrote", out, os.path.getsize(out), "bytes")
