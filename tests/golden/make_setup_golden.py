"""Records tests/golden/setup_parent.npz: every array of every case of tests/setup_bits_cases.py (its SHA-256 above 4 096
entries) as the library in use computes it on an MI355X, and the SHA-256 of every case's inputs. Run ONCE, with the build of
the commit BEFORE a change to the level elimination (csrc/setup_gj.hpp); tests/test_gpu_setup_bits.py then holds the changed
build to these bits. The cases module may be newer than that commit: build the earlier library beside the tree and select it
with MI355SCHUR_LIB, as tools/setup_time.py does for A/B builds —

    git archive HEAD~ julia-phd-krylov-spdes_amd/csrc include | tar -x -C /tmp/parent
    make -C /tmp/parent/julia-phd-krylov-spdes_amd/csrc OUT=$PWD/gpu_jobs/libmi355schur_parent.so
    MI355SCHUR_LIB=$PWD/gpu_jobs/libmi355schur_parent.so python tests/golden/make_setup_golden.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as graft  # noqa: E402
import setup_bits_cases as cases  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "setup_parent.npz")
    pkg = graft.load_package()
    print("library:", pkg._lib.LIB_PATH)
    ctx = pkg.api.Context(0)
    digests = cases.input_digests(pkg.fem)
    results = {}
    for name in cases.NAMES:
        results[name] = cases.run_case(pkg.api, ctx, pkg.fem, name)
        big = sum(a.size > cases.HASH_ABOVE for a in results[name].values())
        print(f"{name}: {len(results[name])} arrays, {big} of them by SHA-256", flush=True)
    np.savez_compressed(out, **cases.pack(results, digests))
    print("wrote", out, os.path.getsize(out), "bytes")
