"""Closed-loop weight sweep on one MI355X: S weight settings x V start poses on a recorded path as ONE ClosedLoop of S * V vehicles.

Every vehicle carries its setting in its own parameter record (BatchMPC.problem_params, `params=`), `run()` runs the episode without a host round trip
and scores every state on the device (kmpc_track_score_batch); the record is downloaded once at the end.  Prints the settings ranked by the rms
cross-track error (mean over the start poses) with the largest |e_ct|, the settle time and the number of non-Optimal solves.
Default draw: C_y (= C_x), C_psi and C_ddf log-uniform within a factor e^SPREAD around the launch file's weights (mpc_cmd_pub.jl:49).

usage: python tools/closed_loop_sweep.py [--settings 256] [--poses 16] [--steps 150] [--path path1_decimated.npz] [--target-vel 5.0] [--spread 1.5]
                                         [--settle-tol 0.5] [--seed 0] [--top 10]
"""
import argparse
import time

import numpy as np
import torch

import _timing as T
from mkz_mpc_path_follower_amd import ClosedLoop  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator  # noqa: E402
import scenario as S  # noqa: E402

N = 8


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--settings", type=int, default=256)
    ap.add_argument("--poses", type=int, default=16)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--path", default="path1_decimated.npz")
    ap.add_argument("--target-vel", type=float, default=5.0)
    ap.add_argument("--spread", type=float, default=1.5)
    ap.add_argument("--settle-tol", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--top", type=int, default=10)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    grt, tr = T.single_path(N, a.path)
    nS, nV = a.settings, a.poses
    settings = np.array(S.WEIGHTS)[None, :].repeat(nS, 0)
    settings[1:, [1, 2, 5]] *= np.exp(rng.uniform(-a.spread, a.spread, (nS - 1, 3)))   # setting 0 stays the launch file's
    settings[:, 0] = settings[:, 1]
    k = rng.integers(0, int(0.5 * len(tr)), nV)
    start = np.stack([tr[k, 4] + rng.uniform(-1, 1, nV), tr[k, 5] + rng.uniform(-1, 1, nV), tr[k, 3] + rng.uniform(-0.2, 0.2, nV)], 1)
    rows = np.tile(start, (nS, 1))                                                    # vehicle s * V + v: setting s from pose v
    sim = VehicleSimulator(nS * nV, X0=rows[:, 0], Y0=rows[:, 1], Psi0=rows[:, 2])
    sim.state[:, 3] = 0.5 * a.target_vel
    loop = ClosedLoop(grt, sim, N=N, target_vel=a.target_vel, weights=S.WEIGHTS)
    par = loop.mpc.problem_params(nS * nV)
    par[:, 0:8] = torch.as_tensor(np.repeat(settings, nV, axis=0), device=par.device)
    loop.params = par
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop.run(a.steps, settle_tol=a.settle_tol)
    sm = loop.score_summary()
    dt = time.perf_counter() - t0
    per = lambda key, f: f(sm[key].reshape(nS, nV), axis=1)
    rms = np.sqrt(per("sum_ect2", np.sum) / per("n", np.sum))
    order = np.argsort(rms)
    print("%s: %d settings x %d start poses = %d vehicles, %d periods at %.1f m/s in %.2f s (%.2f M vehicle-steps/s, one download)"
          % (a.path, nS, nV, nS * nV, a.steps, a.target_vel, dt, nS * nV * a.steps / dt / 1e6))
    print("rank setting      C_y    C_psi    C_ddf   rms e_ct  max|e_ct|  settle s  non-Optimal  refused")
    show = list(order[:a.top]) + ([0] if 0 not in order[:a.top] else [])
    for s in show:
        print("%4d %7d %8.3f %8.3f %8.1f %10.4f %10.4f %9.1f %12d %8d%s"
              % (int(np.where(order == s)[0][0]) + 1, s, settings[s, 1], settings[s, 2], settings[s, 5], rms[s], per("max_ect", np.max)[s],
                 per("t_settle", np.max)[s], per("n_nonopt", np.sum)[s], per("n_refused", np.sum)[s], "   <- the launch file's weights" if s == 0 else ""))
    grt.close()


if __name__ == "__main__":
    main()
