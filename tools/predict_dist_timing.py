"""Timing of the prediction ahead under estimated disturbances (kmpc_predict_ahead_dist_batch) next to the prediction whose steps it extends
(kmpc_predict_ahead_batch), and of the closed loop with observer= and compensator= together, on one MI355X (-> profiles/predict_dist_timing.txt).

  1. One call of kmpc_predict_ahead_batch and of kmpc_predict_ahead_dist_batch at B = 4096 and B = 262 144, 35 serial Euler steps per vehicle
     (command delay 25 updates, fix one period old), on observer records in mid-run.
  2. ClosedLoop vehicle-steps per second at B = 4096, N = 8 on path1 behind a sensor, the plant's command queue and the sensor's stale fix at the
     same 0.35 s: observer= with LatencyCompensator(disturbances=True), observer= alone and estimator= with the plain compensator.
Method: tools/_timing.py.

No target is set: the figure to compare against is the existing stage of the same build in the same process.

usage: python tools/predict_dist_timing.py [out.txt]
"""
import ctypes as C
import sys

import numpy as np
import torch

import _timing as T
from _timing import med, say
from mkz_mpc_path_follower_amd import _lib  # noqa: E402
from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import DisturbanceObserver, Estimator, LatencyCompensator, SensorModel, VehicleSimulator  # noqa: E402

REPS = 100
CMD_DELAY, MEAS_DELAY = 25, 1


def kernels():
    L = _lib.load()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    say("1. us per call, %d steps per vehicle, median [min, max] of %d repeats of %d back-to-back launches" % (10 * MEAS_DELAY + CMD_DELAY, T.REPEATS, REPS))
    for B in (4096, 262144):
        rng = np.random.default_rng(B)
        z = np.stack([rng.uniform(-500, 500, B), rng.uniform(-500, 500, B), rng.uniform(-3, 3, B), rng.uniform(4, 12, B)], 1)
        z = torch.as_tensor(z, device="cuda")
        u = torch.as_tensor(np.stack([np.zeros(B), rng.uniform(-0.1, 0.1, B)], 1), device="cuda")
        ob = DisturbanceObserver(B)
        comp = LatencyCompensator(B, cmd_delay=CMD_DELAY, meas_delay=MEAS_DELAY, disturbances=True)
        comp.cmd_hist.copy_(torch.as_tensor(np.stack([rng.uniform(-1, 1, (comp.depth, B)), rng.uniform(-0.3, 0.3, (comp.depth, B))], 2), device="cuda"))
        est = torch.empty((B, 4), dtype=torch.float64, device="cuda")
        out = torch.empty((B, 4), dtype=torch.float64, device="cuda")
        for _ in range(5):                    # records in mid-run, with disturbance estimates that are not zero
            ob.update(z, u, out=est)
        a = (comp.depth, 100, 10, p(comp.cmd_delay), p(comp.meas_delay), comp.max_cmd_delay, comp.max_meas_delay, 1.108, 1.742)
        run = {
            "kmpc_predict_ahead_batch": lambda: L.kmpc_predict_ahead_batch(0, B, p(est), p(comp.cmd_hist), *a, p(out), None),
            "kmpc_predict_ahead_dist_batch": lambda: L.kmpc_predict_ahead_dist_batch(0, B, p(ob.record), p(est), p(comp.cmd_hist), *a, 0.2, p(out), None),
        }
        for k, fn in run.items():
            assert fn() == 0, k
        res = T.rotate({k: (fn, REPS) for k, fn in run.items()})
        torch.cuda.synchronize()
        assert torch.isfinite(out).all().item()
        for k in run:
            say("   B = %-7d %-32s %8.1f [%8.1f, %8.1f]" % ((B, k) + med(res[k])))


def loops(B=4096, N=8, vt=6.0, steps=100):
    say("2. ClosedLoop, B = %d, N = %d, path1 at %.0f m/s behind a sensor (sigma 0.2, 0.2, 0.01, 0.1), command queue of %d updates, fix %d period old, "
        "%d periods per repeat after 20 warm-up periods, alternating: M vehicle-steps/s (median [min, max] of %d)" % (B, N, vt, CMD_DELAY, MEAS_DELAY, steps, T.REPEATS))
    grt, tr = T.single_path(N)
    start = T.scatter(tr, B, np.random.default_rng(2))
    delays = dict(cmd_delay=CMD_DELAY, meas_delay=MEAS_DELAY)

    def make(kind):
        sim = VehicleSimulator(B, X0=start[:, 0], Y0=start[:, 1], Psi0=start[:, 2], cmd_delay=CMD_DELAY, cmd_queue_depth=4)
        sim.state[:, 3] = vt
        sensor = SensorModel(B, sigma=(0.2, 0.2, 0.01, 0.1), seed=1, meas_delay=MEAS_DELAY)
        if kind == "observer= + compensator=":
            kw = dict(observer=DisturbanceObserver(B, q_dist=(0.0005, 0.0005, 0.005)), compensator=LatencyCompensator(B, disturbances=True, **delays),
                      estimator_input="history")
        elif kind == "observer= alone":
            kw = dict(observer=DisturbanceObserver(B, q_dist=(0.0005, 0.0005, 0.005)))
        else:
            kw = dict(estimator=Estimator.from_sensor(sensor), compensator=LatencyCompensator(B, **delays), estimator_input="history")
        return ClosedLoop(grt, sim, N=N, target_vel=vt, sensor=sensor, **kw)
    kinds = ("estimator= + compensator=", "observer= alone", "observer= + compensator=")
    res, _ = T.loop_rates(kinds, make, B, steps)
    for k in kinds:
        say("   %-28s %6.2f [%6.2f, %6.2f]" % ((k,) + med(res[k])))


def main():
    say(T.header())
    kernels()
    loops()
    T.finish(sys.argv)


if __name__ == "__main__":
    main()
