"""Timing of the measurement stage with sensor faults and of the closed loop with it on one MI355X (-> profiles/sensor_fault_timing.txt).

  1. kmpc_sense_faults_batch (neutral rows; rows with chains, windows and outliers; with a ring of depth 3) next to kmpc_sense_batch and
     kmpc_sense_delayed_batch on the same states at B = 4096 and B = 262 144; then the ratios of the medians.
  2. ClosedLoop vehicle-steps per second at B = 4096, N = 8 on path1: the plain sensor + estimator, and the same with a neutral faulty sensor;
     then the ratio.
Method: tools/_timing.py.  No threshold is set: the stage moves about 0.5 KB per vehicle and is about 1 % of a period.

usage: python tools/sensor_fault_timing.py [out.txt]
"""
import ctypes as C
import sys

import numpy as np
import torch

import _timing as T
from _timing import med, say
from mkz_mpc_path_follower_amd import _lib  # noqa: E402
from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import Estimator, SensorModel, VehicleSimulator, fault_params  # noqa: E402

REPS = 100


def kernels():
    L = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    say("1. us per call, median [min, max] of %d repeats of %d back-to-back launches" % (T.REPEATS, REPS))
    for B in (4096, 262144):
        rng = np.random.default_rng(B)
        s0 = np.zeros((B, 8))
        s0[:, 0:2] = rng.uniform(-500, 500, (B, 2)); s0[:, 2] = rng.uniform(-np.pi, np.pi, B); s0[:, 3] = rng.uniform(4, 12, B)
        s0 = torch.as_tensor(s0, device="cuda")
        sensor = torch.as_tensor(np.tile([0.2, 0.2, 0.01, 0.1, 0.0, 0.0, 0.0, 0.0], (B, 1)), device="cuda")
        est = torch.empty((B, 4), dtype=torch.float64, device="cuda")
        age = torch.as_tensor(rng.integers(0, 3, B), dtype=torch.int32, device="cuda")
        ring = {k: s0[:, 0:4].repeat(3, 1, 1).contiguous() for k in ("plain", "faults")}
        neutral = fault_params(B)
        busy = fault_params(B, p_lose=0.1, p_regain=0.3, win_from_gps=rng.integers(0, 200, B).astype(float), win_len_gps=20.0, p_outlier=0.05,
                            outlier_sigma=3.0, max_age=30.0)
        rec = {k: torch.zeros((B, 16), dtype=torch.float64, device="cuda") for k in ("neutral", "busy", "ring")}
        z, held = torch.empty_like(est), torch.empty_like(est)
        flags, blind = torch.empty((B,), dtype=torch.int32, device="cuda"), torch.empty((B,), dtype=torch.uint8, device="cuda")
        per = [0]

        def faulty(rows, r, with_ring):
            def call():
                per[0] += 1
                return L.kmpc_sense_faults_batch(0, B, p(s0), p(sensor), p(rows), 1, per[0], 0, p(age) if with_ring else None,
                                                 p(ring["faults"]) if with_ring else None, 3, p(r), p(z), p(held), p(flags), p(blind), None)
            return call
        run = {"kmpc_sense_batch": lambda: L.kmpc_sense_batch(0, B, p(s0), p(sensor), 1, 100, 0, p(est), None),
               "kmpc_sense_faults_batch, neutral rows": faulty(neutral, rec["neutral"], False),
               "kmpc_sense_faults_batch, busy rows": faulty(busy, rec["busy"], False),
               "kmpc_sense_delayed_batch": lambda: L.kmpc_sense_delayed_batch(0, B, p(s0), p(sensor), 1, 100, 0, p(age), p(ring["plain"]), 3, p(est), None),
               "kmpc_sense_faults_batch, neutral, ring": faulty(neutral, rec["ring"], True)}
        for k, fn in run.items():
            assert fn() == 0, k
        res = T.rotate({k: (fn, REPS) for k, fn in run.items()})
        assert torch.isfinite(est).all().item() and torch.isfinite(held).all().item() and int(rec["busy"][:, 9].sum().item()) > 0
        for k in run:
            say("   B = %-7d %-40s %8.1f [%8.1f, %8.1f]" % ((B, k) + med(res[k])))
        m = {k: med(v)[0] for k, v in res.items()}
        say("   B = %-7d ratios of the medians: neutral / kmpc_sense_batch %.2f, busy / kmpc_sense_batch %.2f, with a ring / kmpc_sense_delayed_batch %.2f"
            % (B, m["kmpc_sense_faults_batch, neutral rows"] / m["kmpc_sense_batch"], m["kmpc_sense_faults_batch, busy rows"] / m["kmpc_sense_batch"],
               m["kmpc_sense_faults_batch, neutral, ring"] / m["kmpc_sense_delayed_batch"]))


def loops(B=4096, N=8, vt=8.0, steps=100):
    say("2. ClosedLoop, B = %d, N = %d, path1 at %.0f m/s, sensor + estimator, %d periods per repeat after 20 warm-up periods, alternating: M vehicle-steps/s "
        "(median [min, max] of %d)" % (B, N, vt, steps, T.REPEATS))
    grt, tr = T.single_path(N)
    start = T.scatter(tr, B, np.random.default_rng(2))

    def make(kind):
        sim = VehicleSimulator(B, X0=start[:, 0], Y0=start[:, 1], Psi0=start[:, 2], cmd_delay=0)
        sim.state[:, 3] = vt
        sensor = SensorModel(B, sigma=(0.1, 0.1, 0.005, 0.05), seed=1, faults=fault_params(B) if kind == "neutral faulty sensor" else None)
        return ClosedLoop(grt, sim, N=N, target_vel=vt, sensor=sensor, estimator=Estimator.from_sensor(sensor))
    kinds = ("plain sensor", "neutral faulty sensor")
    res, _ = T.loop_rates(kinds, make, B, steps)
    for k in kinds:
        say("   %-36s %6.2f [%6.2f, %6.2f]" % ((k,) + med(res[k])))
    say("   ratio of the medians, neutral faulty sensor / plain sensor: %.3f" % (med(res[kinds[1]])[0] / med(res[kinds[0]])[0]))


def main():
    say(T.header())
    kernels()
    loops()
    T.finish(sys.argv)


if __name__ == "__main__":
    main()
