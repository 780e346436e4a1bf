"""Timing of the ordered leader search (include/kmpc_order.h) against the pair searches on one MI355X (-> profiles/order_timing.txt).

  1. Per call at B = 4096, 32768 and 262144 on the dense fleet of tools/_timing.py (the three fixture paths, ids interleaved, random poses; the
     arclengths and cross-track errors are the track score's): kmpc_order_fleet alone; the ordered follower (kmpc_order_fleet +
     kmpc_order_follow_fleet) against kmpc_follow_fleet; the ordered lane step (kmpc_order_fleet + kmpc_order_lane_step_fleet: tables and
     searches, lanes_max = 2) against kmpc_lane_step_fleet on two lanes in three populations -- everyone in lane 0, one vehicle in 64 in lane 1,
     half and half.  The records' HOLD_LEFT is set far ahead, so that nobody decides a change and a population stays what it is over the
     repeats; every search still runs.  The calls go through the Python host, so launch overhead is in -- the ordered path is a few dozen
     launches.  Before the timing the two searches' outputs are compared once, word for word.
  2. Vehicle-steps per second of ONE ClosedLoop of 32768 vehicles (the platoons of eight of tools/_timing.py) with lanes= on two lanes under
     search="pairs" and search="sorted".
Method: tools/_timing.py; both searches come from the same build.  The pair-search kernels are the parent's code.

usage: python tools/order_timing.py [out.txt]
"""
import sys

import numpy as np
import torch

import _timing as T
from _timing import med, say
from mkz_mpc_path_follower_amd._stage import ptr, stream  # noqa: E402
from mkz_mpc_path_follower_amd.ref_traj import Follower, Lanes, lane_params  # noqa: E402

N, PLATOON = T.N, T.PLATOON
WINS = {}      # stage -> the sizes at which the ordered search took less time


def bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def kernels(B, reps):
    rng = np.random.default_rng(1)
    fleet, state = T.dense_fleet(B, rng)
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
    cases = {"order": (lambda: order_alone(fo), reps), "follow, pairs": (follow(False), reps), "follow, sorted": (follow(True), reps)}
    for name, la in stages:
        cases[name, "pairs"], cases[name, "sorted"] = (lane_step(la, False), reps), (lane_step(la, True), reps)
    t = {k: med(v) for k, v in T.rotate(cases).items()}
    t_fp, t_fo = t["follow, pairs"], t["follow, sorted"]
    say("   B = %d (%d vehicles with a leader; the two searches' outputs equal word for word: %s), %d calls per repeat:"
        % (B, int((fo.leader >= 0).sum().item()), all(same), reps))
    say("     kmpc_order_fleet alone:                                              %10.1f [%10.1f, %10.1f]" % t["order"])
    say("     kmpc_follow_fleet (pair search):                                     %10.1f [%10.1f, %10.1f]" % t_fp)
    say("     kmpc_order_fleet + kmpc_order_follow_fleet:                          %10.1f [%10.1f, %10.1f]   %.3f x the pair search"
        % (t_fo + (t_fo[0] / t_fp[0],)))
    if t_fo[0] < t_fp[0]:
        WINS.setdefault("follower", []).append(B)
    for name, _ in stages:
        t_lp, t_lo = t[name, "pairs"], t[name, "sorted"]
        say("     two lanes, %s:" % name)
        say("       kmpc_lane_step_fleet (pair search):                                %10.1f [%10.1f, %10.1f]" % t_lp)
        say("       kmpc_order_fleet + kmpc_order_lane_step_fleet (tables, searches):  %10.1f [%10.1f, %10.1f]   %.3f x the pair search"
            % (t_lo + (t_lo[0] / t_lp[0],)))
        if t_lo[0] < t_lp[0]:
            WINS.setdefault("lane step, " + name, []).append(B)
        else:
            WINS.setdefault("lane step, " + name, [])
    WINS.setdefault("follower", [])


_SETUP = {}


def make_loop(B, search):
    if B not in _SETUP:                # one waypoint helper for every loop: setting up thousands of paths takes longer than the loops run
        _SETUP[B] = T.platoons(B, B // PLATOON)
    fleet, state = _SETUP[B]
    return T.platoon_loop(fleet, state, lanes=Lanes(fleet, lane_rows=lane_params(B, n_lanes=2), search=search))


def last_step(loop, o):
    return int(o["status"].max().item()), int(loop.lanes.summary()["n_changes"].sum())


def loops(B=32768, steps=50):
    res, last = T.loop_rates(["pairs", "sorted"], lambda search: make_loop(B, search), B, steps, advance=T.step_periods, after=last_step)
    say("2. ClosedLoop of %d vehicles in %d platoons of %d with lanes= (two lanes), N = %d, %d steps per repeat after 20 warm-up steps: M vehicle-steps/s "
        "(median [min, max] of %d, the two searches alternating)" % (B, B // PLATOON, PLATOON, N, steps, T.REPEATS))
    for search in res:
        say("   search=%-10r %6.2f [%6.2f, %6.2f]   (worst status of the last step: %d; lane changes: %d)" % ((search,) + med(res[search]) + last[search][-1]))
    say("   ratio of the medians, sorted / pairs: %.3f" % (med(res["sorted"])[0] / med(res["pairs"])[0]))


def main():
    say(T.header())
    say("1. per call, us (median [min, max] of %d repeats; device events around back-to-back calls through the Python host)" % T.REPEATS)
    kernels(4096, 100)
    kernels(32768, 30)
    kernels(262144, 5)
    say("   the smallest of the three sizes at which the ordered search takes less time than the pair search:")
    for stage, sizes in WINS.items():
        say("     %-50s %s" % (stage + ":", min(sizes) if sizes else "none of them"))
    loops()
    T.finish(sys.argv)


if __name__ == "__main__":
    main()
