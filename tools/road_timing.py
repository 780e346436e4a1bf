"""Timing of the plant with a road row (kmpc_sim_advance_road) next to the queue kernel it copies, and of the closed loop with it, on one MI355X
(-> profiles/road_timing.txt).

  1. One control period (10 updates = 100 sub-steps, depth 2, no delay) of kmpc_sim_advance_queue, of kmpc_sim_advance_road with the neutral row and
     of kmpc_sim_advance_road with two saturating rows -- mu_f = 0.2 alone (the front axle runs out of grip, the vehicle understeers and its slip
     angles stay inside the plant kernels' polynomial range: what the clip itself costs) and mu = 0.2 on both axles with a bank of 0.5 m/s^2 and an
     offset of 0.03 rad (the rear lets go as well, vehicles slide and the wave takes the library's atan2) -- and of the neutral row without
     road_stat, at B = 4096 and B = 262 144; the share of clipped sub-steps and the largest slip tangent at the end are printed.  Device events
     around REPS launches after a warm-up, the kernels in rotation inside one process, five repeats each, median and range.  Every variant restarts from the same states in every repeat.
  2. ClosedLoop vehicle-steps per second at B = 4096, N = 8 on path1 with VehicleSimulator(cmd_queue_depth=2) and with road=road_params(B, mu=0.5),
     alternating, median of five.

No target is set: the figure to compare against is the queue kernel of the same build in the same process.

usage: python tools/road_timing.py [out.txt]
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
from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator, plant_params, road_params  # noqa: E402

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
    say("1. us per control period, median [min, max] of %d repeats of %d back-to-back launches" % (REPEATS, REPS))
    for B in (4096, 262144):
        rng = np.random.default_rng(B)
        s0 = np.zeros((B, 8))
        s0[:, 0:2] = rng.uniform(-500, 500, (B, 2)); s0[:, 2] = rng.uniform(-np.pi, np.pi, B); s0[:, 3] = rng.uniform(4, 12, B)
        s0[:, 4] = rng.uniform(-0.1, 0.1, B); s0[:, 5] = rng.uniform(-0.1, 0.1, B); s0[:, 7] = rng.uniform(-0.1, 0.1, B)
        s0 = torch.as_tensor(s0, device="cuda")
        # the command holds the speed and keeps steering: the states stay in the polynomials' ranges over the 103 periods of a repeat
        cmd = torch.as_tensor(np.stack([np.zeros(B), rng.uniform(-0.1, 0.1, B)], 1), device="cuda")
        rows = plant_params(B)
        neutral, front, slippery = road_params(B), road_params(B, mu_f=0.2), road_params(B, mu=0.2, a_lat=0.5, df_offset=0.03)
        names = ("kmpc_sim_advance_queue", "kmpc_sim_advance_road, neutral row", "kmpc_sim_advance_road, neutral row, no road_stat",
                 "kmpc_sim_advance_road, front axle saturating", "kmpc_sim_advance_road, both axles saturating")
        st = {k: s0.clone() for k in names}
        qu = {k: cmd.repeat(2, 1, 1).contiguous() for k in names}
        stat = {k: torch.zeros((B, 4), dtype=torch.float64, device="cuda") for k in names}
        per = {k: 0 for k in names}

        def road_call(k, road, with_stat=True):
            def fn():
                per[k] += 1
                return L.kmpc_sim_advance_road(0, B, p(st[k]), p(cmd), p(rows), p(road), None, p(qu[k]), 2, per[k], 10, p(stat[k]) if with_stat else None, None)
            return fn

        def queue_call():
            k = names[0]
            per[k] += 1
            return L.kmpc_sim_advance_queue(0, B, p(st[k]), p(cmd), p(rows), None, p(qu[k]), 2, per[k], 10, None)
        run = {names[0]: queue_call, names[1]: road_call(names[1], neutral), names[2]: road_call(names[2], neutral, False),
               names[3]: road_call(names[3], front), names[4]: road_call(names[4], slippery)}
        for k, fn in run.items():
            assert fn() == 0, k
        res = {k: [] for k in run}
        for _ in range(REPEATS):
            for k in names:
                st[k].copy_(s0); stat[k].zero_()
            for k, fn in run.items():   # in rotation
                res[k].append(event_time(fn, REPS))
        torch.cuda.synchronize()
        assert all(torch.isfinite(t).all().item() for t in st.values())
        assert torch.equal(st[names[0]], st[names[1]]) and torch.equal(st[names[0]], st[names[2]]) and not stat[names[1]].any().item()
        for k in names:
            say("   B = %-7d %-50s %8.1f [%8.1f, %8.1f]" % ((B, k) + med(res[k])))
        say("   B = %-7d neutral row = the queue kernel's states bit for bit after %d periods" % (B, REPS + 3))
        for k in names[3:]:
            sat = stat[k][:, 0:2].sum(0) / (B * 100.0 * (REPS + 3))
            tan = ((st[k][:, 4].abs() + 1.152 * st[k][:, 5].abs()) / st[k][:, 3]).max().item()
            say("   B = %-7d %s: %.0f %% of the front and %.0f %% of the rear sub-steps clipped, largest (|vy| + lf |wz|) / vx at the end %.3f "
                "(the slip-angle polynomial holds to 0.125)" % (B, k.split(", ")[1], 100.0 * sat[0].item(), 100.0 * sat[1].item(), tan))


def loops(B=4096, N=8, vt=6.0, steps=100):
    say("2. ClosedLoop, B = %d, N = %d, path1 at %.0f m/s, %d periods per repeat after 20 warm-up periods, alternating: M vehicle-steps/s "
        "(median [min, max] of %d)" % (B, N, vt, steps, REPEATS))
    d = np.load(os.path.join(ROOT, "tests", "golden", "path1_decimated.npz"))
    grt = GPSRefTrajectory(arrays=dict(t=d["t"], lat=d["lat"], lon=d["lon"], psi=d["psi"]), traj_horizon=N, traj_dt=0.2)
    tr = grt.get_global_trajectory_reference()
    rng = np.random.default_rng(2)
    idx = rng.integers(0, int(0.5 * len(tr)), B)
    X0, Y0, P0 = tr[idx, 4] + rng.uniform(-0.5, 0.5, B), tr[idx, 5] + rng.uniform(-0.5, 0.5, B), tr[idx, 3] + rng.uniform(-0.05, 0.05, B)

    def make(kind):
        if kind == "cmd_queue_depth=2":
            sim = VehicleSimulator(B, X0=X0, Y0=Y0, Psi0=P0, cmd_queue_depth=2)
        else:
            sim = VehicleSimulator(B, X0=X0, Y0=Y0, Psi0=P0, road=road_params(B, mu=0.5))
        sim.state[:, 3] = vt
        return ClosedLoop(grt, sim, N=N, target_vel=vt)
    kinds = ("cmd_queue_depth=2", "road=road_params(B, mu=0.5)")
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
        say("   %-36s %6.2f [%6.2f, %6.2f]" % ((k,) + med(res[k])))


def main():
    say("%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    kernels()
    loops()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
