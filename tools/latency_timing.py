"""Timing of the latency stages and of the closed loop with them on one MI355X (-> profiles/latency_timing.txt).

  1. kmpc_sim_advance_queue (one control period, depth 4, delays 0 ... 30) next to kmpc_sim_advance_plant with a delay, kmpc_sense_delayed_batch
     (depth 3) next to kmpc_sense_batch, kmpc_cmd_in_force_batch, and kmpc_predict_ahead_batch at 35, 50 and 80 serial Euler steps per vehicle,
     at B = 4096 and B = 262 144; the plant states restart from the same values in every repeat.
  2. ClosedLoop vehicle-steps per second at B = 4096, N = 8 on path1: sensor + estimator, and the same with a command queue (delay 25 updates), a fix
     one period old and the compensator (35 steps of prediction per vehicle and period).
Method: tools/_timing.py.

usage: python tools/latency_timing.py [out.txt]
"""
import ctypes as C
import sys

import numpy as np
import torch

import _timing as T
from _timing import med, say
from mkz_mpc_path_follower_amd import _lib  # noqa: E402
from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import Estimator, LatencyCompensator, SensorModel, VehicleSimulator, plant_params  # noqa: E402

REPS = 100


def kernels():
    L = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    say("1. us per call, median [min, max] of %d repeats of %d back-to-back launches" % (T.REPEATS, REPS))
    for B in (4096, 262144):
        rng = np.random.default_rng(B)
        s0 = np.zeros((B, 8))
        s0[:, 0:2] = rng.uniform(-500, 500, (B, 2)); s0[:, 2] = rng.uniform(-np.pi, np.pi, B); s0[:, 3] = rng.uniform(4, 12, B)
        s0[:, 7] = rng.uniform(-0.05, 0.05, B)
        s0 = torch.as_tensor(s0, device="cuda")
        cmd = torch.as_tensor(np.stack([rng.uniform(-0.2, 0.2, B), rng.uniform(-0.05, 0.05, B)], 1), device="cuda")
        rows, held = plant_params(B), cmd.clone()
        delay1 = torch.as_tensor(rng.integers(0, 11, B), dtype=torch.int32, device="cuda")
        delay3 = torch.as_tensor(rng.integers(0, 31, B), dtype=torch.int32, device="cuda")
        queue = cmd.repeat(4, 1, 1).contiguous()
        sensor = torch.as_tensor(np.tile([0.2, 0.2, 0.01, 0.1, 0.0, 0.0, 0.0, 0.0], (B, 1)), device="cuda")
        est = torch.empty((B, 4), dtype=torch.float64, device="cuda")
        age = torch.as_tensor(rng.integers(0, 3, B), dtype=torch.int32, device="cuda")
        ring = s0[:, 0:4].repeat(3, 1, 1).contiguous()
        z = s0[:, 0:4].contiguous()
        zo, uo = torch.empty_like(z), torch.empty((B, 2), dtype=torch.float64, device="cuda")
        hist = cmd.repeat(9, 1, 1).contiguous()
        full = lambda v: torch.full((B,), v, dtype=torch.int32, device="cuda")
        d25, d30, l1, l2, l5 = full(25), full(30), full(1), full(2), full(5)
        st = {k: s0.clone() for k in ("plant", "queue")}
        per = [100]   # a period late enough for every delay to reach back into the log

        def queue_call():
            per[0] += 1
            return L.kmpc_sim_advance_queue(0, B, p(st["queue"]), p(cmd), p(rows), p(delay3), p(queue), 4, per[0], 10, None)
        run = {"kmpc_sim_advance_plant + delay": lambda: L.kmpc_sim_advance_plant(0, B, p(st["plant"]), p(cmd), p(rows), p(delay1), p(held), 10, None),
               "kmpc_sim_advance_queue": queue_call,
               "kmpc_sense_batch": lambda: L.kmpc_sense_batch(0, B, p(s0), p(sensor), 1, 100, 0, p(est), None),
               "kmpc_sense_delayed_batch": lambda: L.kmpc_sense_delayed_batch(0, B, p(s0), p(sensor), 1, 100, 0, p(age), p(ring), 3, p(est), None),
               "kmpc_cmd_in_force_batch": lambda: L.kmpc_cmd_in_force_batch(0, B, p(hist), 9, 100, 10, p(d25), p(l1), 30, 5, p(uo), None),
               "kmpc_predict_ahead_batch, 35 steps": lambda: L.kmpc_predict_ahead_batch(0, B, p(z), p(hist), 9, 100, 10, p(d25), p(l1), 30, 5, 1.108, 1.742, p(zo), None),
               "kmpc_predict_ahead_batch, 50 steps": lambda: L.kmpc_predict_ahead_batch(0, B, p(z), p(hist), 9, 100, 10, p(d30), p(l2), 30, 5, 1.108, 1.742, p(zo), None),
               "kmpc_predict_ahead_batch, 80 steps": lambda: L.kmpc_predict_ahead_batch(0, B, p(z), p(hist), 9, 100, 10, p(d30), p(l5), 30, 5, 1.108, 1.742, p(zo), None)}
        for k, fn in run.items():
            assert fn() == 0, k
        res = T.rotate({k: (fn, REPS) for k, fn in run.items()}, before=lambda: [t.copy_(s0) for t in st.values()])
        assert all(torch.isfinite(t).all().item() for t in (st["plant"], st["queue"], est, zo, uo))
        for k in run:
            say("   B = %-7d %-36s %8.1f [%8.1f, %8.1f]" % ((B, k) + med(res[k])))


def loops(B=4096, N=8, vt=8.0, steps=100):
    say("2. ClosedLoop, B = %d, N = %d, path1 at %.0f m/s, %d periods per repeat after 20 warm-up periods, alternating: M vehicle-steps/s "
        "(median [min, max] of %d)" % (B, N, vt, steps, T.REPEATS))
    grt, tr = T.single_path(N)
    start = T.scatter(tr, B, np.random.default_rng(2))

    def make(kind):
        if kind == "sensor + estimator":
            sim = VehicleSimulator(B, X0=start[:, 0], Y0=start[:, 1], Psi0=start[:, 2], cmd_delay=0)
            sim.state[:, 3] = vt
            sensor = SensorModel(B, sigma=(0.1, 0.1, 0.005, 0.05), seed=1)
            return ClosedLoop(grt, sim, N=N, target_vel=vt, sensor=sensor, estimator=Estimator.from_sensor(sensor))
        sim = VehicleSimulator(B, X0=start[:, 0], Y0=start[:, 1], Psi0=start[:, 2], cmd_delay=25, cmd_queue_depth=4)
        sim.state[:, 3] = vt
        sensor = SensorModel(B, sigma=(0.1, 0.1, 0.005, 0.05), seed=1, meas_delay=1)
        return ClosedLoop(grt, sim, N=N, target_vel=vt, sensor=sensor, estimator=Estimator.from_sensor(sensor), estimator_input="history",
                          compensator=LatencyCompensator(B, cmd_delay=25, meas_delay=1))
    kinds = ("sensor + estimator", "+ queue, stale fix, compensator")
    res, _ = T.loop_rates(kinds, make, B, steps)
    for k in kinds:
        say("   %-36s %6.2f [%6.2f, %6.2f]" % ((k,) + med(res[k])))


def main():
    say(T.header())
    kernels()
    loops()
    T.finish(sys.argv)


if __name__ == "__main__":
    main()
