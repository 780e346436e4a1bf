"""Timing of the prediction ahead under estimated disturbances (kmpc_predict_ahead_dist_batch) next to the prediction whose steps it extends
(kmpc_predict_ahead_batch), and of the closed loop with observer= and compensator= together, on one MI355X (-> profiles/predict_dist_timing.txt).

  1. One call of kmpc_predict_ahead_batch and of kmpc_predict_ahead_dist_batch at B = 4096 and B = 262 144, 35 serial Euler steps per vehicle
     (command delay 25 updates, fix one period old), on observer records in mid-run.  tools/observer_timing.py's method: device events around REPS
     launches after a warm-up, the kernels in rotation inside one process, five repeats each, median and range.
  2. ClosedLoop vehicle-steps per second at B = 4096, N = 8 on path1 behind a sensor, the plant's command queue and the sensor's stale fix at the
     same 0.35 s: observer= with LatencyCompensator(disturbances=True), observer= alone and estimator= with the plain compensator, alternating,
     median of five.

No target is set: the figure to compare against is the existing stage of the same build in the same process.

usage: python tools/predict_dist_timing.py [out.txt]
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
from mkz_mpc_path_follower_amd.vehicle_sim import DisturbanceObserver, Estimator, LatencyCompensator, SensorModel, VehicleSimulator  # noqa: E402

REPEATS, REPS = 5, 100
CMD_DELAY, MEAS_DELAY = 25, 1
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
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    say("1. us per call, %d steps per vehicle, median [min, max] of %d repeats of %d back-to-back launches" % (10 * MEAS_DELAY + CMD_DELAY, REPEATS, REPS))
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
        res = {k: [] for k in run}
        for _ in range(REPEATS):
            for k, fn in run.items():   # in rotation
                res[k].append(event_time(fn, REPS))
        torch.cuda.synchronize()
        assert torch.isfinite(out).all().item()
        for k in run:
            say("   B = %-7d %-32s %8.1f [%8.1f, %8.1f]" % ((B, k) + med(res[k])))


def loops(B=4096, N=8, vt=6.0, steps=100):
    say("2. ClosedLoop, B = %d, N = %d, path1 at %.0f m/s behind a sensor (sigma 0.2, 0.2, 0.01, 0.1), command queue of %d updates, fix %d period old, "
        "%d periods per repeat after 20 warm-up periods, alternating: M vehicle-steps/s (median [min, max] of %d)" % (B, N, vt, CMD_DELAY, MEAS_DELAY, steps, REPEATS))
    d = np.load(os.path.join(ROOT, "tests", "golden", "path1_decimated.npz"))
    grt = GPSRefTrajectory(arrays=dict(t=d["t"], lat=d["lat"], lon=d["lon"], psi=d["psi"]), traj_horizon=N, traj_dt=0.2)
    tr = grt.get_global_trajectory_reference()
    rng = np.random.default_rng(2)
    idx = rng.integers(0, int(0.5 * len(tr)), B)
    X0, Y0, P0 = tr[idx, 4] + rng.uniform(-0.5, 0.5, B), tr[idx, 5] + rng.uniform(-0.5, 0.5, B), tr[idx, 3] + rng.uniform(-0.05, 0.05, B)
    delays = dict(cmd_delay=CMD_DELAY, meas_delay=MEAS_DELAY)

    def make(kind):
        sim = VehicleSimulator(B, X0=X0, Y0=Y0, Psi0=P0, cmd_delay=CMD_DELAY, cmd_queue_depth=4)
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
        say("   %-28s %6.2f [%6.2f, %6.2f]" % ((k,) + med(res[k])))


def main():
    say("%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    kernels()
    loops()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
