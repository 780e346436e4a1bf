"""Timing of the Gauss-Markov stage and of the closed loop with it on one MI355X (-> profiles/wander_timing.txt).

  1. kmpc_wander_batch (neutral rows: no draw; busy rows: all eight channels on; both with both pairs composed) next to kmpc_sense_faults_batch
     (neutral rows), the nearest stage in bytes moved, on the same build at B = 4096 and B = 262 144; then the bytes each call must move, counted from the shapes,
     over the median time.
       kmpc_wander_batch         reads  wander 192 + record 128 + two base rows 64 + 64, writes record 128 + two rows 64 + 64      = 704 B / vehicle
       kmpc_sense_faults_batch   reads  state 32 (of a 64-byte row) + sensor 64 + faults 120 + record 128, writes record 128 + z 32
                                 + held 32 + flags 4 + blind 1                                                                    = 541 B / vehicle
  2. ClosedLoop vehicle-steps per second at B = 4096, N = 8 on path1 with a sensor, an estimator and a road: without wander= and with it (coloured
     GPS error and a gust); then the ratio.
Method: tools/_timing.py.  No threshold is set.

usage: python tools/wander_timing.py [out.txt]
"""
import ctypes as C
import sys

import numpy as np
import torch

import _timing as T
from _timing import med, say
from mkz_mpc_path_follower_amd import _lib  # noqa: E402
from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import Estimator, SensorModel, VehicleSimulator, Wander, fault_params, road_params, wander_params  # noqa: E402

REPS = 100
WANDER_BYTES, FAULTS_BYTES = 704, 541


def kernels():
    L = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    say("1. us per call, median [min, max] of %d repeats of %d back-to-back launches; then GB/s = the bytes the call must move / the median" % (T.REPEATS, REPS))
    for B in (4096, 262144):
        rng = np.random.default_rng(B)
        s0 = np.zeros((B, 8))
        s0[:, 0:2] = rng.uniform(-500, 500, (B, 2)); s0[:, 2] = rng.uniform(-np.pi, np.pi, B); s0[:, 3] = rng.uniform(4, 12, B)
        s0 = torch.as_tensor(s0, device="cuda")
        sensor = torch.as_tensor(np.tile([0.2, 0.2, 0.01, 0.1, 0.0, 0.0, 0.0, 0.0], (B, 1)), device="cuda")
        road = road_params(B, mu=0.9, a_lat=0.3)
        sensor_out, road_out = torch.empty_like(sensor), torch.empty_like(road)
        rows = {"neutral": wander_params(B), "busy": wander_params(B, sigma=(0.2, 0.2, 0.01, 0.05, 0.3, 0.5, 0.005, 1.0), tau=(10, 10, 5, 0, 2, 2, 30, 1))}
        wrec = {k: torch.zeros((B, 16), dtype=torch.float64, device="cuda") for k in rows}
        faults, frec = fault_params(B), torch.zeros((B, 16), dtype=torch.float64, device="cuda")
        z, held = torch.empty((B, 4), dtype=torch.float64, device="cuda"), torch.empty((B, 4), dtype=torch.float64, device="cuda")
        flags, blind = torch.empty((B,), dtype=torch.int32, device="cuda"), torch.empty((B,), dtype=torch.uint8, device="cuda")
        per = [0]

        def wander(kind):
            def call():
                per[0] += 1
                return L.kmpc_wander_batch(0, B, p(rows[kind]), p(wrec[kind]), 1, per[0], 0, p(sensor), p(sensor_out), p(road), p(road_out), None)
            return call

        def faulty():
            per[0] += 1
            return L.kmpc_sense_faults_batch(0, B, p(s0), p(sensor), p(faults), 1, per[0], 0, None, None, 0, p(frec), p(z), p(held), p(flags), p(blind), None)
        run = {"kmpc_wander_batch, neutral rows": (wander("neutral"), WANDER_BYTES), "kmpc_wander_batch, busy rows": (wander("busy"), WANDER_BYTES),
               "kmpc_sense_faults_batch, neutral rows": (faulty, FAULTS_BYTES)}
        for k, (fn, _) in run.items():
            assert fn() == 0, k
        res = T.rotate({k: (fn, REPS) for k, (fn, _) in run.items()})
        assert torch.isfinite(wrec["busy"]).all().item() and (wrec["busy"][:, 0:8] != 0).all().item() and not wrec["neutral"][:, 0:8].any().item()
        assert torch.equal(sensor_out[:, 0:4], sensor[:, 0:4]) and torch.isfinite(held).all().item()
        for k, (_, nbytes) in run.items():
            m = med(res[k])
            say("   B = %-7d %-40s %8.1f [%8.1f, %8.1f]   %7.1f GB/s" % ((B, k) + m + (B * nbytes / (m[0] * 1e-6) / 1e9,)))
        m = {k: med(v)[0] for k, v in res.items()}
        say("   B = %-7d ratios of the medians to kmpc_sense_faults_batch: neutral %.2f, busy %.2f" %
            (B, m["kmpc_wander_batch, neutral rows"] / m["kmpc_sense_faults_batch, neutral rows"],
             m["kmpc_wander_batch, busy rows"] / m["kmpc_sense_faults_batch, neutral rows"]))


def loops(B=4096, N=8, vt=8.0, steps=100):
    say("2. ClosedLoop, B = %d, N = %d, path1 at %.0f m/s, sensor + estimator + road, %d periods per repeat after 20 warm-up periods, alternating: M vehicle-steps/s "
        "(median [min, max] of %d)" % (B, N, vt, steps, T.REPEATS))
    grt, tr = T.single_path(N)
    start = T.scatter(tr, B, np.random.default_rng(2))

    def make(kind):
        sim = VehicleSimulator(B, X0=start[:, 0], Y0=start[:, 1], Psi0=start[:, 2], road=road_params(B))
        sim.state[:, 3] = vt
        sensor = SensorModel(B, sigma=(0.1, 0.1, 0.005, 0.05), seed=1)
        kw = {}
        if kind == "with wander=":
            kw["wander"] = Wander(B, wander_params(B, sigma=(0.2, 0.2, 0, 0, 0, 0.5, 0, 0), tau=(10, 10, 0, 0, 0, 2, 0, 0)), seed=1)
        return ClosedLoop(grt, sim, N=N, target_vel=vt, sensor=sensor, estimator=Estimator.from_sensor(sensor), **kw)
    kinds = ("without wander=", "with wander=")
    res, _ = T.loop_rates(kinds, make, B, steps)
    for k in kinds:
        say("   %-36s %6.2f [%6.2f, %6.2f]" % ((k,) + med(res[k])))
    say("   ratio of the medians, with / without: %.3f" % (med(res[kinds[1]])[0] / med(res[kinds[0]])[0]))


def main():
    say(T.header())
    kernels()
    loops()
    T.finish(sys.argv)


if __name__ == "__main__":
    main()
