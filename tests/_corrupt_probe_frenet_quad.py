"""Child process of test_frenet_quad.py::test_slack_guard_trips_in_the_frenet_quad_kernel: loads the TEST build libkmpc_hip_corrupt.so (csrc/Makefile:
one thread's slack iterate is pushed 1e-3 off b - a_f^T U after the second accepted step) in place of the shipped library, solves a Frenet batch at N = 8
with kernel_variant = 3 (four problems per wave) and prints the status counts as JSON."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from mkz_mpc_path_follower_amd import _lib  # noqa: E402

_lib.LIB_PATH = os.path.join(ROOT, "mkz_mpc_path_follower_amd", "libkmpc_hip_corrupt.so")
from mkz_mpc_path_follower_amd import BatchMPC  # noqa: E402
from test_frenet import _cases  # noqa: E402

z0, kp, vt, up = _cases(64, 8, seed=36)
o = BatchMPC(N=8, dtype=torch.float64, model=1, kernel_variant=3).solve_frenet(z0, kp, vt, up)
torch.cuda.synchronize()
st = o["status"].cpu().numpy()
print("CORRUPT_PROBE " + json.dumps({"quad_frenet_f64_N8": [int((st == k).sum()) for k in range(4)]}))
