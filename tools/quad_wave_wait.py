"""How long a finished row of the four-problems-per-wave Frenet kernel (kernel_variant = 3) waits for its wave: mean and maximum iteration count per
problem against per wave (the wave runs until its last row is done), from the `iters` output of one draw alone.  usage: quad_wave_wait.py [B] [seed]"""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from mkz_mpc_path_follower_amd import BatchMPC
from test_frenet import _cases
B = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 3
z0, kp, vt, up = _cases(B, 8, seed)
s = BatchMPC(N=8, dtype=torch.float64, model=1, kernel_variant=3)
o = s.solve_frenet(z0, kp, vt, up, want_U=True)
for tag in ("cold", "warm"):
    it = o["iters"].cpu().numpy().astype(np.int64)
    st = o["status"].cpu().numpy()
    w = it[:B - B % 4].reshape(-1, 4).max(1)   # index order: wave i holds problems 4i .. 4i+3
    print("%s B=%d seed=%d: per problem mean %.3f max %d; per wave mean %.3f max %d; rows idle %.1f %% of the wave's iterations; status!=0: %d" % (
        tag, B, seed, it.mean(), it.max(), w.mean(), w.max(), 100.0 * (1.0 - it[:B - B % 4].mean() / w.mean()), int((st != 0).sum())))
    if tag == "cold":
        o = s.solve_frenet(z0, kp, vt, up, warm_U=o["U"].clone(), warm=True, want_U=True)
