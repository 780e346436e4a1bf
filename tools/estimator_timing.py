"""Timing of the state estimator and of the closed loop with it on one MI355X (-> profiles/estimator_timing.txt).

  1. one call of kmpc_estimate_batch (records in mid-run; with and without innov / flags outputs) next to kmpc_sense_batch on the same states at
     B = 4096 and B = 262 144.
  2. ClosedLoop vehicle-steps per second at B = 4096, N = 8 on path1 with a sensor, with and without the estimator stage, from the same run.
Method: tools/_timing.py.

usage: python tools/estimator_timing.py [out.txt]
"""
import ctypes as C
import sys

import numpy as np
import torch

import _timing as T
from _timing import med, say
from mkz_mpc_path_follower_amd import _lib  # noqa: E402
from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import Estimator, SensorModel, VehicleSimulator  # noqa: E402

REPS = 100
SIGMA = (0.2, 0.2, 0.01, 0.1)


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
        sensor = torch.as_tensor(np.tile(SIGMA + (0.0, 0.0, 0.0, 0.0), (B, 1)), device="cuda")
        z = torch.empty((B, 4), dtype=torch.float64, device="cuda")
        assert L.kmpc_sense_batch(0, B, p(s0), p(sensor), 1, 0, 0, p(z), None) == 0
        est = Estimator(B, r=SIGMA)
        est.update(z, s0[:, 6:8])          # initialised: the timed calls predict and update (z stays: the record settles, the work per call does not change)
        out = torch.empty((B, 4), dtype=torch.float64, device="cuda")
        u = C.c_void_p(s0.data_ptr() + 48)
        args = (0, B, p(est.record), p(z), u, 8, p(est.params), 0.1, est.L_a, est.L_b, 0.0, p(out))
        run = {"kmpc_sense_batch": lambda: L.kmpc_sense_batch(0, B, p(s0), p(sensor), 1, 0, 0, p(z), None),
               "kmpc_estimate_batch": lambda: L.kmpc_estimate_batch(*args, None, None, None),
               "kmpc_estimate_batch + innov, flags": lambda: L.kmpc_estimate_batch(*args, p(est.innov), p(est.flags), None)}
        res = T.rotate({k: (fn, REPS) for k, fn in run.items()})
        assert torch.isfinite(est.record).all().item() and not (est.flags & 32).any().item()
        for k in run:
            say("   B = %-7d %-36s %8.1f [%8.1f, %8.1f]" % ((B, k) + med(res[k])))


def loops(B=4096, N=8, vt=8.0, steps=100):
    say("2. ClosedLoop, B = %d, N = %d, path1 at %.0f m/s, sensor sigma %s, %d periods per repeat after 20 warm-up periods: M vehicle-steps/s "
        "(median [min, max] of %d)" % (B, N, vt, SIGMA, steps, T.REPEATS))
    grt, tr = T.single_path(N)
    start = T.scatter(tr, B, np.random.default_rng(2))

    def make(kind):
        sim = VehicleSimulator(B, X0=start[:, 0], Y0=start[:, 1], Psi0=start[:, 2])
        sim.state[:, 3] = vt
        sensor = SensorModel(B, sigma=SIGMA, seed=1)
        return ClosedLoop(grt, sim, N=N, target_vel=vt, sensor=sensor, estimator=Estimator.from_sensor(sensor) if kind == "sensor + estimator" else None)
    kinds = ("sensor", "sensor + estimator")
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
