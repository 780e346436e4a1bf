"""Timing of the per-vehicle plant kernel and of the Monte-Carlo closed loop on one MI355X (-> profiles/plant_sensor_timing.txt).

  1. one control period (10 model updates = 100 sub-steps) of kmpc_sim_advance_plant (default rows; with and without a command delay) against
     kmpc_sim_advance_batch at B = 4096 and B = 262 144, and kmpc_sense_batch on the same states; the plant states restart from the same values
     in every repeat.
  2. ClosedLoop vehicle-steps per second at B = 4096, N = 8 on path1 with sensor + plant rows + delay, next to the plain loop's from the same run.
Method: tools/_timing.py.

usage: python tools/plant_timing.py [out.txt]
"""
import ctypes as C
import sys

import numpy as np
import torch

import _timing as T
from _timing import med, say
from mkz_mpc_path_follower_amd import _lib  # noqa: E402
from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import SensorModel, VehicleSimulator, plant_params  # noqa: E402

REPS = 100


def kernels():
    L = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    say("1. us per control period (10 updates), median [min, max] of %d repeats of %d back-to-back launches" % (T.REPEATS, REPS))
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
        res = T.rotate({k: (fn, REPS) for k, fn in run.items()}, before=lambda: [t.copy_(s0) for t in st.values()])
        assert torch.equal(st["fixed"], st["plant"]) and torch.isfinite(st["delay"]).all().item()
        for k in run:
            say("   B = %-7d %-32s %8.1f [%8.1f, %8.1f]" % ((B, k) + med(res[k])))


def loops(B=4096, N=8, vt=8.0, steps=100):
    say("2. ClosedLoop, B = %d, N = %d, path1 at %.0f m/s, %d periods per repeat after 20 warm-up periods: M vehicle-steps/s (median [min, max] of %d)"
        % (B, N, vt, steps, T.REPEATS))
    grt, tr = T.single_path(N)
    rng = np.random.default_rng(2)
    start = T.scatter(tr, B, rng)
    rows = dict(m=1840.0 * rng.uniform(0.8, 1.3, B), C_alpha_f=4.0703e4 * rng.uniform(0.7, 1.2, B), C_alpha_r=6.4495e4 * rng.uniform(0.7, 1.2, B))

    def make(kind):
        if kind == "plain":
            sim = VehicleSimulator(B, X0=start[:, 0], Y0=start[:, 1], Psi0=start[:, 2])
            sim.state[:, 3] = vt
            return ClosedLoop(grt, sim, N=N, target_vel=vt)
        sim = VehicleSimulator(B, X0=start[:, 0], Y0=start[:, 1], Psi0=start[:, 2], plant=plant_params(B, **rows), cmd_delay=rng.integers(0, 6, B))
        sim.state[:, 3] = vt
        return ClosedLoop(grt, sim, N=N, target_vel=vt, sensor=SensorModel(B, sigma=(0.1, 0.1, 0.005, 0.05), seed=1))
    kinds = ("plain", "sensor + plant rows + delay")
    res, _ = T.loop_rates(kinds, make, B, steps)
    for k in kinds:
        say("   %-32s %6.2f [%6.2f, %6.2f]" % ((k,) + med(res[k])))


def main():
    say(T.header())
    kernels()
    loops()
    T.finish(sys.argv)


if __name__ == "__main__":
    main()
