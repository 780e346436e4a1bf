"""Timing of the ordered leader search (include/kmpc_order.h) against the pair searches on one MI355X (-> profiles/order_timing.txt).

  1. Per call at B = 4096, 32768 and 262144 on tools/lanes_timing.py's dense fleet (the three fixture paths, ids interleaved, random poses; the
     arclengths and cross-track errors are the track score's): kmpc_order_fleet alone; the ordered follower (kmpc_order_fleet +
     kmpc_order_follow_fleet) against kmpc_follow_fleet; the ordered lane step (kmpc_order_fleet + kmpc_order_lane_step_fleet: tables and
     searches, lanes_max = 2) against kmpc_lane_step_fleet on two lanes in three populations -- everyone in lane 0, one vehicle in 64 in lane 1,
     half and half.  The records' HOLD_LEFT is set far ahead, so that nobody decides a change and a population stays what it is over the
     repeats; every search still runs.  Device events around REPS back-to-back calls through the Python host, so launch overhead is in -- the
     ordered path is a few dozen launches.  Before the timing the two searches' outputs are compared once, word for word.
  2. Vehicle-steps per second of ONE ClosedLoop of 32768 vehicles (tools/follow_timing.py's platoons of eight) with lanes= on two lanes under
     search="pairs" and search="sorted".
Method of tools/follow_timing.py: both searches come from the same build and alternate inside one process, five repeats
each, median and range.  The pair-search kernels are the parent's code.

usage: python tools/order_timing.py [out.txt]
"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import follow_timing as FT  # noqa: E402  (puts the tree and tests/ on the path)
from mkz_mpc_path_follower_amd import ClosedLoop, FleetRefTrajectory  # noqa: E402
from mkz_mpc_path_follower_amd._stage import ptr, stream  # noqa: E402
from mkz_mpc_path_follower_amd.ref_traj import Follower, Lanes, lane_params  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator  # noqa: E402

REPEATS, N = FT.REPEATS, FT.N
say, med, event_time = FT.say, FT.med, FT.event_time
WINS = {}      # stage -> the sizes at which the ordered search took less time


def bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def kernels(B, reps):
    rng = np.random.default_rng(1)
    paths = [FT.path_dict(f) for f in FT.FILES]
    pid = np.arange(B) % 3
    fleet = FleetRefTrajectory(paths, pid, traj_horizon=N)
    state = np.zeros((B, 8))
    for p, tr in enumerate(fleet.trajectories):
        sel = np.where(pid == p)[0]
        idx = rng.integers(0, int(0.6 * len(tr)), len(sel))
        state[sel, 0], state[sel, 1], state[sel, 2] = tr[idx, 4] + rng.uniform(-1, 1, len(sel)), tr[idx, 5] + rng.uniform(-1, 1, len(sel)), tr[idx, 3]
    state[:, 3] = rng.uniform(2.0, 8.0, B)
    st = torch.as_tensor(state, device="cuda")
    vt = torch.full((B,), 6.0, dtype=torch.float64, device="cuda")
    dev = torch.device("cuda", 0)
    lib, sm = fleet._lib, stream(dev)
    out = torch.empty((B,), dtype=torch.float64, device="cuda")
    fo = Follower(fleet, search="sorted")
    fo.cap(st, vt, out=out)
    err = fo._track["err"]
    head = (0, B, ptr(err[:, 3]), 4, ptr(st[:, 3]), 8, ptr(fleet.path_id), None)

    def order_alone(o):
        lib.kmpc_order_fleet(*head, ptr(o.order), ptr(o._count), ptr(o._ws), o._ws.numel(), sm)

    def follow(ordered):
        def call():
            tail = (ptr(fo.rows), ptr(vt), ptr(out), ptr(fo.gap_leader), ptr(fo.leader), ptr(fo.stat))
            if ordered:
                order_alone(fo)
                lib.kmpc_order_follow_fleet(*head, *tail, ptr(fo.order), sm)
            else:
                lib.kmpc_follow_fleet(*head, *tail, sm)
        return call

    def lane_step(la, ordered, count=[0]):
        def call():
            k = count[0] = count[0] + 1
            args = (0, B, k, 0.1, ptr(err[:, 3]), 4, ptr(err[:, 0]), 4, ptr(st[:, 3]), 8, ptr(fleet.path_id), None, ptr(la.follow_rows),
                    ptr(la.rows), ptr(vt), ptr(out), ptr(la._occ[k % 2]), ptr(la._occ[1 - k % 2]), ptr(la.rec), ptr(la.gap_leader), ptr(la.leader),
                    ptr(la.neighbours))
            if ordered:
                order_alone(la)
                lib.kmpc_order_lane_step_fleet(*args, ptr(la.order), la.lanes_max, ptr(la._ws), la._ws.numel(), sm)
            else:
                lib.kmpc_lane_step_fleet(*args, sm)
        return call

    def snapshot(call, tensors):
        call()
        torch.cuda.synchronize()
        return [bits(t).clone() for t in tensors]

    pops = [("everyone in lane 0", np.zeros(B, dtype=np.int64)), ("one vehicle in 64 in lane 1", (rng.random(B) < 1.0 / 64).astype(np.int64)),
            ("half in lane 0, half in lane 1", rng.integers(0, 2, B))]
    stages = []
    for name, lane0 in pops:
        la = Lanes(fleet, lane_rows=lane_params(B, n_lanes=2), lane0=lane0, search="sorted")
        la.rec[:, 3] = 1e9            # HOLD_LEFT: nobody decides, the population stays
        for k in range(2):            # both occupancy buffers written
            la.step(st, vt, k, 0.1, out=out)
        stages.append((name, la))
    # the two searches' outputs, once, word for word (the record runs on: compared are the words a call writes from the inputs alone)
    a = snapshot(follow(False), (out, fo.gap_leader, fo.leader))
    b = snapshot(follow(True), (out, fo.gap_leader, fo.leader))
    same = [all(torch.equal(x, y) for x, y in zip(a, b))]
    for _, la in stages:
        outs = (out, la.gap_leader, la.leader, la.neighbours)
        a = snapshot(lane_step(la, False), outs)
        b = snapshot(lane_step(la, True), outs)
        same.append(all(torch.equal(x, y) for x, y in zip(a, b)))
    t_o, t_fp, t_fo = [], [], []
    t_lp, t_lo = [[] for _ in stages], [[] for _ in stages]
    for _ in range(REPEATS):   # alternating
        t_o.append(event_time(lambda: order_alone(fo), reps))
        t_fp.append(event_time(follow(False), reps))
        t_fo.append(event_time(follow(True), reps))
        for i, (_, la) in enumerate(stages):
            t_lp[i].append(event_time(lane_step(la, False), reps))
            t_lo[i].append(event_time(lane_step(la, True), reps))
    say("   B = %d (%d vehicles with a leader; the two searches' outputs equal word for word: %s), %d calls per repeat:"
        % (B, int((fo.leader >= 0).sum().item()), all(same), reps))
    say("     kmpc_order_fleet alone:                                              %10.1f [%10.1f, %10.1f]" % med(t_o))
    say("     kmpc_follow_fleet (pair search):                                     %10.1f [%10.1f, %10.1f]" % med(t_fp))
    say("     kmpc_order_fleet + kmpc_order_follow_fleet:                          %10.1f [%10.1f, %10.1f]   %.3f x the pair search"
        % (med(t_fo) + (med(t_fo)[0] / med(t_fp)[0],)))
    if med(t_fo)[0] < med(t_fp)[0]:
        WINS.setdefault("follower", []).append(B)
    for i, (name, _) in enumerate(stages):
        say("     two lanes, %s:" % name)
        say("       kmpc_lane_step_fleet (pair search):                                %10.1f [%10.1f, %10.1f]" % med(t_lp[i]))
        say("       kmpc_order_fleet + kmpc_order_lane_step_fleet (tables, searches):  %10.1f [%10.1f, %10.1f]   %.3f x the pair search"
            % (med(t_lo[i]) + (med(t_lo[i])[0] / med(t_lp[i])[0],)))
        if med(t_lo[i])[0] < med(t_lp[i])[0]:
            WINS.setdefault("lane step, " + name, []).append(B)
        else:
            WINS.setdefault("lane step, " + name, [])
    WINS.setdefault("follower", [])


_SETUP = {}


def loop_rate(B, search, steps):
    if B not in _SETUP:                # one waypoint helper for every loop: setting up thousands of paths takes longer than the loops run
        _SETUP[B] = FT.setup(B, B // FT.PLATOON)
    fleet, state = _SETUP[B]
    sim = VehicleSimulator(B, X0=state[:, 0], Y0=state[:, 1], Psi0=state[:, 2])
    sim.state[:, 3] = 6.0
    loop = ClosedLoop(fleet, sim, N=N, target_vel=6.0, lanes=Lanes(fleet, lane_rows=lane_params(B, n_lanes=2), search=search))
    for _w in range(20):
        loop.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _s in range(steps):
        o = loop.step()
    torch.cuda.synchronize()
    rate = B * steps / (time.perf_counter() - t0) / 1e6
    return rate, int(o["status"].max().item()), int(loop.lanes.summary()["n_changes"].sum())


def loops(B=32768, steps=50):
    res, last = {"pairs": [], "sorted": []}, {}
    for _ in range(REPEATS):
        for search in res:
            r = loop_rate(B, search, steps)
            res[search].append(r[0])
            last[search] = r[1:]
    say("2. ClosedLoop of %d vehicles in %d platoons of %d with lanes= (two lanes), N = %d, %d steps per repeat after 20 warm-up steps: M vehicle-steps/s "
        "(median [min, max] of %d, the two searches alternating)" % (B, B // FT.PLATOON, FT.PLATOON, N, steps, REPEATS))
    for search in res:
        say("   search=%-10r %6.2f [%6.2f, %6.2f]   (worst status of the last step: %d; lane changes: %d)" % ((search,) + med(res[search]) + last[search]))
    say("   ratio of the medians, sorted / pairs: %.3f" % (med(res["sorted"])[0] / med(res["pairs"])[0]))


def main():
    say("%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    say("1. per call, us (median [min, max] of %d repeats; device events around back-to-back calls through the Python host)" % REPEATS)
    kernels(4096, 100)
    kernels(32768, 30)
    kernels(262144, 5)
    say("   the smallest of the three sizes at which the ordered search takes less time than the pair search:")
    for stage, sizes in WINS.items():
        say("     %-50s %s" % (stage + ":", min(sizes) if sizes else "none of them"))
    loops()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(FT.LINES) + "\n")


if __name__ == "__main__":
    main()
