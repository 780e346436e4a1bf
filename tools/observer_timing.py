"""Timing of the disturbance observer (kmpc_observe_batch) next to the estimator whose filter it extends (kmpc_estimate_batch), of the command
offset (kmpc_cmd_offset_batch), and of the closed loop with either stage, on one MI355X (-> profiles/observer_timing.txt).

  1. One call of kmpc_estimate_batch (128 B record), of kmpc_observe_batch (320 B record) with all outputs and with est_out alone, and of
     kmpc_cmd_offset_batch, at B = 4096 and B = 262 144, on records in mid-run.  The bytes a call must move (record in and out, row, z, u, outputs)
     are printed next to the time.
  2. ClosedLoop vehicle-steps per second at B = 4096, N = 8 on path1 behind a sensor, with estimator= and with observer=.
Method: tools/_timing.py.

No target is set: the figure to compare against is the estimator of the same build in the same process.

usage: python tools/observer_timing.py [out.txt]
"""
import ctypes as C
import sys

import numpy as np
import torch

import _timing as T
from _timing import med, say
from mkz_mpc_path_follower_amd import _lib  # noqa: E402
from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import DisturbanceObserver, Estimator, SensorModel, VehicleSimulator  # noqa: E402

REPS = 100


def kernels():
    L = _lib.load()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    say("1. us per call, median [min, max] of %d repeats of %d back-to-back launches; bytes moved per vehicle and the bandwidth that median means" % (T.REPEATS, REPS))
    for B in (4096, 262144):
        rng = np.random.default_rng(B)
        z = np.stack([rng.uniform(-500, 500, B), rng.uniform(-500, 500, B), rng.uniform(-3, 3, B), rng.uniform(4, 12, B)], 1)
        z = torch.as_tensor(z, device="cuda")
        u = torch.as_tensor(np.stack([np.zeros(B), rng.uniform(-0.1, 0.1, B)], 1), device="cuda")   # the speed holds: the records stay in mid-run
        est, ob = Estimator(B), DisturbanceObserver(B)
        cmd = torch.zeros((B, 2), dtype=torch.float64, device="cuda")
        out = torch.empty((B, 4), dtype=torch.float64, device="cuda")
        for _ in range(5):                    # past the first call: every timed call predicts and updates
            est.update(z, u, out=out); ob.update(z, u, out=out)
        run = {
            "kmpc_estimate_batch": (lambda: L.kmpc_estimate_batch(0, B, p(est.record), p(z), p(u), 2, p(est.params), 0.1, 1.108, 1.742, 0.0, p(out), p(est.innov),
                                                                   p(est.flags), None), 2 * 128 + 64 + 32 + 16 + 32 + 32 + 4),
            "kmpc_observe_batch": (lambda: L.kmpc_observe_batch(0, B, p(ob.record), p(z), p(u), 2, p(ob.params), 0.1, 1.108, 1.742, 0.0, 1.0, 0.2, p(out), p(ob.dist),
                                                                 p(ob.innov), p(ob.flags), None), 2 * 320 + 128 + 32 + 16 + 32 + 24 + 32 + 4),
            "kmpc_observe_batch, est_out alone": (lambda: L.kmpc_observe_batch(0, B, p(ob.record), p(z), p(u), 2, p(ob.params), 0.1, 1.108, 1.742, 0.0, 1.0, 0.2,
                                                                                p(out), None, None, None, None), 2 * 320 + 128 + 32 + 16 + 32),
            "kmpc_cmd_offset_batch": (lambda: L.kmpc_cmd_offset_batch(0, B, p(ob.record), None, 0.5, 0.1, p(cmd), None), 3 * 64 + 32),   # three 64 B sectors of the record
        }
        for k, (fn, _) in run.items():
            assert fn() == 0, k
        res = T.rotate({k: (fn, REPS) for k, (fn, _) in run.items()})
        torch.cuda.synchronize()
        assert torch.isfinite(est.record).all().item() and torch.isfinite(ob.record).all().item() and not (ob.flags & 32).any().item()
        for k, (_, nbytes) in run.items():
            m = med(res[k])
            say("   B = %-7d %-36s %8.1f [%8.1f, %8.1f]   %4d B   %7.1f GB/s" % ((B, k) + m + (nbytes, B * nbytes / m[0] / 1e3)))


def loops(B=4096, N=8, vt=6.0, steps=100):
    say("2. ClosedLoop, B = %d, N = %d, path1 at %.0f m/s behind a sensor (sigma 0.2, 0.2, 0.01, 0.1), %d periods per repeat after 20 warm-up periods, "
        "alternating: M vehicle-steps/s (median [min, max] of %d)" % (B, N, vt, steps, T.REPEATS))
    grt, tr = T.single_path(N)
    start = T.scatter(tr, B, np.random.default_rng(2))

    def make(kind):
        sim = VehicleSimulator(B, X0=start[:, 0], Y0=start[:, 1], Psi0=start[:, 2])
        sim.state[:, 3] = vt
        sensor = SensorModel(B, sigma=(0.2, 0.2, 0.01, 0.1), seed=1)
        kw = dict(estimator=Estimator.from_sensor(sensor)) if kind == "estimator=" else dict(observer=DisturbanceObserver(B)) if kind == "observer=" else {}
        return ClosedLoop(grt, sim, N=N, target_vel=vt, sensor=sensor, **kw)
    kinds = ("sensor alone", "estimator=", "observer=")
    res, _ = T.loop_rates(kinds, make, B, steps)
    for k in kinds:
        say("   %-16s %6.2f [%6.2f, %6.2f]" % ((k,) + med(res[k])))


def main():
    say(T.header())
    kernels()
    loops()
    T.finish(sys.argv)


if __name__ == "__main__":
    main()
