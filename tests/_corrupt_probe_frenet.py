"""Child process of test_frenet_wide.py::test_slack_guard_trips_in_the_frenet_four_wave_kernel: loads the TEST build libkmpc_hip_corrupt.so (csrc/Makefile:
one thread's slack iterate is pushed 1e-3 off b - a_f^T U after the second accepted step) in place of the shipped library, solves a Frenet batch at N = 50
(four-wave kernel) and prints the status counts as JSON."""
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
from test_frenet_wide import _long_cases  # noqa: E402

z0, kp, vt, up = _long_cases(64, 50, seed=17)
o = BatchMPC(N=50, dtype=torch.float64, model=1).solve_frenet(z0, kp, vt, up)
torch.cuda.synchronize()
st = o["status"].cpu().numpy()
print("CORRUPT_PROBE " + json.dumps({"wide_frenet_f64_N50": [int((st == k).sum()) for k in range(4)]}))
