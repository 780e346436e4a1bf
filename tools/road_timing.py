"""Timing of the plant with a road row (kmpc_sim_advance_road) next to the queue kernel it copies, and of the closed loop with it, on one MI355X
(-> profiles/road_timing.txt).

  1. One control period (10 updates = 100 sub-steps, depth 2, no delay) of kmpc_sim_advance_queue, of kmpc_sim_advance_road with the neutral row and
     of kmpc_sim_advance_road with two saturating rows -- mu_f = 0.2 alone (the front axle runs out of grip, the vehicle understeers and its slip
     angles stay inside the plant kernels' polynomial range: what the clip itself costs) and mu = 0.2 on both axles with a bank of 0.5 m/s^2 and an
     offset of 0.03 rad (the rear lets go as well, vehicles slide and the wave takes the library's atan2) -- and of the neutral row without
     road_stat, at B = 4096 and B = 262 144; the share of clipped sub-steps and the largest slip tangent at the end are printed.  Every variant
     restarts from the same states in every repeat.
  2. ClosedLoop vehicle-steps per second at B = 4096, N = 8 on path1 with VehicleSimulator(cmd_queue_depth=2) and with road=road_params(B, mu=0.5).
Method: tools/_timing.py.

No target is set: the figure to compare against is the queue kernel of the same build in the same process.

usage: python tools/road_timing.py [out.txt]
"""
import ctypes as C
import sys

import numpy as np
import torch

import _timing as T
from _timing import med, say
from mkz_mpc_path_follower_amd import _lib  # noqa: E402
from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator, plant_params, road_params  # noqa: E402

REPS = 100


def kernels():
    L = _lib.load()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    say("1. us per control period, median [min, max] of %d repeats of %d back-to-back launches" % (T.REPEATS, REPS))
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
        def restart():
            for k in names:
                st[k].copy_(s0); stat[k].zero_()
        res = T.rotate({k: (fn, REPS) for k, fn in run.items()}, before=restart)
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
        "(median [min, max] of %d)" % (B, N, vt, steps, T.REPEATS))
    grt, tr = T.single_path(N)
    start = T.scatter(tr, B, np.random.default_rng(2))

    def make(kind):
        if kind == "cmd_queue_depth=2":
            sim = VehicleSimulator(B, X0=start[:, 0], Y0=start[:, 1], Psi0=start[:, 2], cmd_queue_depth=2)
        else:
            sim = VehicleSimulator(B, X0=start[:, 0], Y0=start[:, 1], Psi0=start[:, 2], road=road_params(B, mu=0.5))
        sim.state[:, 3] = vt
        return ClosedLoop(grt, sim, N=N, target_vel=vt)
    kinds = ("cmd_queue_depth=2", "road=road_params(B, mu=0.5)")
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
