"""Timing of the per-vehicle plant kernel and of the Monte-Carlo closed loop on one MI355X (-> profiles/plant_sensor_timing.txt).

  1. one control period (10 model updates = 100 sub-steps) of kmpc_sim_advance_plant (default rows; with and without a command delay) against
     kmpc_sim_advance_batch at B = 4096 and B = 262 144, and kmpc_sense_batch on the same states: device events around REPS launches after a warm-up,
     the kernels in rotation inside one process, five repeats each, median and range.
  2. ClosedLoop vehicle-steps per second at B = 4096, N = 8 on path1 with sensor + plant rows + delay, next to the plain loop's from the same run.

usage: python tools/plant_timing.py [out.txt]
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mkz_mpc_path_follower_amd import _lib  # noqa: E402
from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop  # noqa: E402
from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import SensorModel, VehicleSimulator, plant_params  # noqa: E402

REPEATS, REPS = 5, 100
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def event_time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps   # us per call


def kernels():
    L = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    say("1. us per control period (10 updates), median [min, max] of %d repeats of %d back-to-back launches" % (REPEATS, REPS))
    for B in (4096, 262144):
        rng = np.random.default_rng(B)
        s0 = np.zeros((B, 8))
        s0[:, 0:2] = rng.uniform(-500, 500, (B, 2)); s0[:, 2] = rng.uniform(-np.pi, np.pi, B); s0[:, 3] = rng.uniform(4, 12, B)
        s0[:, 7] = rng.uniform(-0.05, 0.05, B)
        s0 = torch.as_tensor(s0, device="cuda")
        cmd = torch.as_tensor(np.stack([rng.uniform(-0.2, 0.2, B), rng.uniform(-0.05, 0.05, B)], 1), device="cuda")
        rows, held = plant_params(B), cmd.clone()
        delay = torch.as_tensor(rng.integers(0, 11, B), dtype=torch.int32, device="cuda")
        sensor = torch.as_tensor(np.tile([0.2, 0.2, 0.01, 0.1, 0.0, 0.0, 0.0, 0.0], (B, 1)), device="cuda")
        est = torch.empty((B, 4), dtype=torch.float64, device="cuda")
        st = {k: s0.clone() for k in ("fixed", "plant", "delay")}
        run = {"kmpc_sim_advance_batch": lambda: L.kmpc_sim_advance_batch(0, B, p(st["fixed"]), p(cmd), 10, None),
               "kmpc_sim_advance_plant": lambda: L.kmpc_sim_advance_plant(0, B, p(st["plant"]), p(cmd), p(rows), None, None, 10, None),
               "kmpc_sim_advance_plant + delay": lambda: L.kmpc_sim_advance_plant(0, B, p(st["delay"]), p(cmd), p(rows), p(delay), p(held), 10, None),
               "kmpc_sense_batch": lambda: L.kmpc_sense_batch(0, B, p(s0), p(sensor), 1, 0, 0, p(est), None)}
        res = {k: [] for k in run}
        for _ in range(REPEATS):
            for t in st.values():
                t.copy_(s0)
            for k, fn in run.items():   # in rotation
                res[k].append(event_time(fn, REPS))
        assert torch.equal(st["fixed"], st["plant"]) and torch.isfinite(st["delay"]).all().item()
        for k in run:
            say("   B = %-7d %-32s %8.1f [%8.1f, %8.1f]" % ((B, k) + med(res[k])))


def loops(B=4096, N=8, vt=8.0, steps=100):
    say("2. ClosedLoop, B = %d, N = %d, path1 at %.0f m/s, %d periods per repeat after 20 warm-up periods: M vehicle-steps/s (median [min, max] of %d)"
        % (B, N, vt, steps, REPEATS))
    d = np.load(os.path.join(ROOT, "tests", "golden", "path1_decimated.npz"))
    grt = GPSRefTrajectory(arrays=dict(t=d["t"], lat=d["lat"], lon=d["lon"], psi=d["psi"]), traj_horizon=N, traj_dt=0.2)
    tr = grt.get_global_trajectory_reference()
    rng = np.random.default_rng(2)
    idx = rng.integers(0, int(0.5 * len(tr)), B)
    X0, Y0, P0 = tr[idx, 4] + rng.uniform(-0.5, 0.5, B), tr[idx, 5] + rng.uniform(-0.5, 0.5, B), tr[idx, 3] + rng.uniform(-0.05, 0.05, B)
    rows = dict(m=1840.0 * rng.uniform(0.8, 1.3, B), C_alpha_f=4.0703e4 * rng.uniform(0.7, 1.2, B), C_alpha_r=6.4495e4 * rng.uniform(0.7, 1.2, B))

    def make(kind):
        if kind == "plain":
            sim = VehicleSimulator(B, X0=X0, Y0=Y0, Psi0=P0)
            sim.state[:, 3] = vt
            return ClosedLoop(grt, sim, N=N, target_vel=vt)
        sim = VehicleSimulator(B, X0=X0, Y0=Y0, Psi0=P0, plant=plant_params(B, **rows), cmd_delay=rng.integers(0, 6, B))
        sim.state[:, 3] = vt
        return ClosedLoop(grt, sim, N=N, target_vel=vt, sensor=SensorModel(B, sigma=(0.1, 0.1, 0.005, 0.05), seed=1))
    kinds = ("plain", "sensor + plant rows + delay")
    res = {k: [] for k in kinds}
    for _ in range(REPEATS):
        for k in kinds:
            loop = make(k)
            loop.run(20, score=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop.run(steps, score=False)
            torch.cuda.synchronize()
            res[k].append(B * steps / (time.perf_counter() - t0) / 1e6)
    for k in kinds:
        say("   %-32s %6.2f [%6.2f, %6.2f]" % ((k,) + med(res[k])))


def main():
    say("%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    kernels()
    loops()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
