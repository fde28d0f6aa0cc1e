"""Records tests/golden/launch_args_parent.npz: x, it and res_norm of every case of tests/launch_args_cases.py, as the
build in the tree computes them on an MI355X. Run ONCE, on the commit BEFORE a change to how the loop kernels take their
arguments; tests/test_gpu_launch_args.py then holds the changed build to these bits.

    python tests/golden/make_launch_args_golden.py [out.npz]
"""
import os
import sys

# the sharded case runs two in-process ranks: same settings as tests/conftest.py, before the first HIP call
if int(os.environ.get("GPU_MAX_HW_QUEUES") or 0) < 16:
    os.environ["GPU_MAX_HW_QUEUES"] = "16"
os.environ.setdefault("GPU_FORCE_BLIT_COPY_SIZE", "1048576")

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as graft  # noqa: E402
import launch_args_cases as cases  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "launch_args_parent.npz")
    api = graft.load_package().api
    results = cases.run_all(api, api.Context(0))
    for name, (x, it, res) in results.items():
        print(f"{name}: n = {x.size} it = {it} res_norm[-1] = {res[-1] if res.size else float('nan'):.3e}")
    np.savez_compressed(out, **cases.pack(results))
    print("wrote", out, os.path.getsize(out), "bytes")
