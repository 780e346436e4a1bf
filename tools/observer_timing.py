"""Timing of the disturbance observer (kmpc_observe_batch) next to the estimator whose filter it extends (kmpc_estimate_batch), of the command
offset (kmpc_cmd_offset_batch), and of the closed loop with either stage, on one MI355X (-> profiles/observer_timing.txt).

  1. One call of kmpc_estimate_batch (128 B record), of kmpc_observe_batch (320 B record) with all outputs and with est_out alone, and of
     kmpc_cmd_offset_batch, at B = 4096 and B = 262 144, on records in mid-run.  Device events around REPS launches after a warm-up, the kernels in
     rotation inside one process, five repeats each, median and range.  The bytes a call must move (record in and out, row, z, u, outputs) are printed
     next to the time.
  2. ClosedLoop vehicle-steps per second at B = 4096, N = 8 on path1 behind a sensor, with estimator= and with observer=, alternating, median of five.

No target is set: the figure to compare against is the estimator of the same build in the same process.

usage: python tools/observer_timing.py [out.txt]
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
from mkz_mpc_path_follower_amd.vehicle_sim import DisturbanceObserver, Estimator, SensorModel, VehicleSimulator  # noqa: E402

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
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    say("1. us per call, median [min, max] of %d repeats of %d back-to-back launches; bytes moved per vehicle and the bandwidth that median means" % (REPEATS, REPS))
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
        res = {k: [] for k in run}
        for _ in range(REPEATS):
            for k, (fn, _) in run.items():   # in rotation
                res[k].append(event_time(fn, REPS))
        torch.cuda.synchronize()
        assert torch.isfinite(est.record).all().item() and torch.isfinite(ob.record).all().item() and not (ob.flags & 32).any().item()
        for k, (_, nbytes) in run.items():
            m = med(res[k])
            say("   B = %-7d %-36s %8.1f [%8.1f, %8.1f]   %4d B   %7.1f GB/s" % ((B, k) + m + (nbytes, B * nbytes / m[0] / 1e3)))


def loops(B=4096, N=8, vt=6.0, steps=100):
    say("2. ClosedLoop, B = %d, N = %d, path1 at %.0f m/s behind a sensor (sigma 0.2, 0.2, 0.01, 0.1), %d periods per repeat after 20 warm-up periods, "
        "alternating: M vehicle-steps/s (median [min, max] of %d)" % (B, N, vt, steps, REPEATS))
    d = np.load(os.path.join(ROOT, "tests", "golden", "path1_decimated.npz"))
    grt = GPSRefTrajectory(arrays=dict(t=d["t"], lat=d["lat"], lon=d["lon"], psi=d["psi"]), traj_horizon=N, traj_dt=0.2)
    tr = grt.get_global_trajectory_reference()
    rng = np.random.default_rng(2)
    idx = rng.integers(0, int(0.5 * len(tr)), B)
    X0, Y0, P0 = tr[idx, 4] + rng.uniform(-0.5, 0.5, B), tr[idx, 5] + rng.uniform(-0.5, 0.5, B), tr[idx, 3] + rng.uniform(-0.05, 0.05, B)

    def make(kind):
        sim = VehicleSimulator(B, X0=X0, Y0=Y0, Psi0=P0)
        sim.state[:, 3] = vt
        sensor = SensorModel(B, sigma=(0.2, 0.2, 0.01, 0.1), seed=1)
        kw = dict(estimator=Estimator.from_sensor(sensor)) if kind == "estimator=" else dict(observer=DisturbanceObserver(B)) if kind == "observer=" else {}
        return ClosedLoop(grt, sim, N=N, target_vel=vt, sensor=sensor, **kw)
    kinds = ("sensor alone", "estimator=", "observer=")
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
        say("   %-16s %6.2f [%6.2f, %6.2f]" % ((k,) + med(res[k])))


def main():
    say("%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    kernels()
    loops()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
