"""Timing of the lane stage on one MI355X (-> profiles/lanes_timing.txt).

  1. kmpc_lane_step_fleet next to kmpc_follow_fleet and kmpc_waypoints_fleet of the same build at B = 4096, 32768 and 262144: the dense fleet of
     tools/_timing.py (the three fixture paths, ids interleaved, random poses) on four lanes, the lanes random, a tenth of the vehicles in mid-change;
     the calls go through the Python host, so launch overhead is in.  The stage is timed as the kernel alone (arclengths and
     cross-track errors given; occupancy ping-ponged, the record running) and as Lanes.step() (the geometry-only score call, the on-the-road mask
     and the kernel).  To see where the time goes the kernel is also timed on ONE lane (the four side searches find no band to test, the scan still
     reads every candidate) -- the difference to kmpc_follow_fleet is then the wider tile and the five-fold compare-and-select, not the winners.
  2. kmpc_ref_offset_batch (Lanes.shift on a [B,9,3] table, every offset non-zero) next to the waypoint call.
  3. vehicle-steps per second of ONE ClosedLoop of 4096 vehicles without a stage, with follower= and with lanes= (two lanes): the 512 platoons of
     eight of tools/_timing.py, so that all three solve the same problems.
Method: tools/_timing.py.

usage: python tools/lanes_timing.py [out.txt]
"""
import sys

import numpy as np
import torch

import _timing as T
from _timing import med, say
from mkz_mpc_path_follower_amd._stage import ptr, stream  # noqa: E402
from mkz_mpc_path_follower_amd.ref_traj import Follower, Lanes, lane_params  # noqa: E402

N, PLATOON = T.N, T.PLATOON


def lanes_on(fleet, B, n_lanes, rng):
    """a lane stage on `fleet` with random lanes in 0 ... n_lanes - 1 and a tenth of the vehicles in mid-change towards a neighbouring lane"""
    lane0 = rng.integers(0, n_lanes, B)
    la = Lanes(fleet, lane_rows=lane_params(B, n_lanes=n_lanes), lane0=lane0)
    if n_lanes > 1:
        rec = la.rec.cpu().numpy()
        mid = rng.random(B) < 0.1
        frm = np.where(lane0 == 0, 1, lane0 - 1)
        rec[mid, 1], rec[mid, 2] = frm[mid], (lane0 * 3.5 + (frm - lane0) * 3.5 * 0.5)[mid]
        la.rec.copy_(torch.from_numpy(rec))
        occ = ((1 << rec[:, 0].astype(np.int64)) | (1 << rec[:, 1].astype(np.int64))).astype(np.uint32).view(np.int32)
        la._occ[la._cur].copy_(torch.from_numpy(occ))
    return la


def kernels(B, reps):
    rng = np.random.default_rng(1)
    fleet, state = T.dense_fleet(B, rng)
    st = torch.as_tensor(state, device="cuda")
    pose = st[:, 0:3].contiguous()
    vt = torch.full((B,), 6.0, dtype=torch.float64, device="cuda")
    dev = torch.device("cuda", 0)
    out = torch.empty((B,), dtype=torch.float64, device="cuda")
    fo = Follower(fleet)
    fo.cap(st, vt, out=out)
    la4, la1 = lanes_on(fleet, B, 4, rng), lanes_on(fleet, B, 1, rng)
    la4.step(st, vt, 0, 0.1, out=out)
    la1.step(st, vt, 0, 0.1, out=out)
    torch.cuda.synchronize()
    nb = la4.neighbours.cpu().numpy()
    found = [int((la4.leader >= 0).sum().item())] + [int(np.isfinite(nb[:, i, 0]).sum()) for i in range(4)]
    err = fo._track["err"]
    ref, _ = fleet.get_waypoints_batch(pose, vt)
    la4.rec[:, 2] += 0.25    # every offset non-zero: every row of the table is shifted
    count = [0]

    def follow_alone():
        fleet._lib.kmpc_follow_fleet(0, B, ptr(err[:, 3]), 4, ptr(st[:, 3]), 8, ptr(fleet.path_id), None, ptr(fo.rows), ptr(vt), ptr(out),
                                     ptr(fo.gap_leader), ptr(fo.leader), ptr(fo.stat), stream(dev))

    def lanes_alone(la):
        def call():
            k = count[0] = count[0] + 1
            fleet._lib.kmpc_lane_step_fleet(0, B, k, 0.1, ptr(err[:, 3]), 4, ptr(err[:, 0]), 4, ptr(st[:, 3]), 8, ptr(fleet.path_id), None,
                                            ptr(la.follow_rows), ptr(la.rows), ptr(vt), ptr(out), ptr(la._occ[k % 2]), ptr(la._occ[1 - k % 2]),
                                            ptr(la.rec), ptr(la.gap_leader), ptr(la.leader), ptr(la.neighbours), stream(dev))
        return call
    t = T.rotate({"waypoints": (lambda: fleet.get_waypoints_batch(pose, vt), reps), "follow": (follow_alone, reps),
                  "four lanes": (lanes_alone(la4), reps), "one lane": (lanes_alone(la1), reps),
                  "step": (lambda: la4.step(st, vt, 2, 0.1, out=out), reps), "shift": (lambda: la4.shift(ref), reps)})
    tw, tf, t4, t1, ts, to = (med(t[k]) for k in ("waypoints", "follow", "four lanes", "one lane", "step", "shift"))
    say("   B = %d (four lanes: %d vehicles with an own-lane leader; left-ahead %d, left-behind %d, right-ahead %d, right-behind %d), %d calls per repeat:"
        % ((B,) + tuple(found) + (reps,)))
    say("     kmpc_waypoints_fleet, target-velocity mode:                  %10.1f [%10.1f, %10.1f]" % tw)
    say("     kmpc_follow_fleet alone (arclengths given):                  %10.1f [%10.1f, %10.1f]" % tf)
    say("     kmpc_lane_step_fleet alone, four lanes:                      %10.1f [%10.1f, %10.1f]   %.3f x kmpc_follow_fleet; %.4f ns per follower-candidate pair"
        % (t4 + (t4[0] / tf[0], t4[0] * 1e3 / (float(B) * B))))
    say("     kmpc_lane_step_fleet alone, one lane:                        %10.1f [%10.1f, %10.1f]   %.3f x kmpc_follow_fleet" % (t1 + (t1[0] / tf[0],)))
    say("     Lanes.step(): score call + on-the-road mask + the kernel:    %10.1f [%10.1f, %10.1f]   %.3f x the waypoint call" % (ts + (ts[0] / tw[0],)))
    say("     kmpc_ref_offset_batch on [B,9,3] (Lanes.shift):              %10.1f [%10.1f, %10.1f]   %.3f x the waypoint call" % (to + (to[0] / tw[0],)))


def make_loop(B, kind):
    fleet, state = T.platoons(B, B // PLATOON)
    kw = {}
    if kind == "follower":
        kw["follower"] = Follower(fleet)
    elif kind == "lanes":
        kw["lanes"] = Lanes(fleet, lane_rows=lane_params(B, n_lanes=2))
    return T.platoon_loop(fleet, state, **kw)


def last_step(loop, o):
    changes = int(loop.lanes.summary()["n_changes"].sum()) if loop.lanes is not None else 0
    return int(o["status"].max().item()), float(o["iters"].double().mean().item()), changes


def loops(B=4096, steps=100):
    kinds = {"without a stage": None, "with follower= (default rows)": "follower", "with lanes= (two lanes)": "lanes"}
    res, last = T.loop_rates(list(kinds), lambda k: make_loop(B, kinds[k]), B, steps, advance=T.step_periods, after=last_step)
    say("2. ClosedLoop of %d vehicles in %d platoons of %d, %g m apart at 6 m/s, N = %d, %d steps per repeat after 20 warm-up steps: M vehicle-steps/s "
        "(median [min, max] of %d, the three loops alternating)" % (B, B // PLATOON, PLATOON, T.SPACING, N, steps, T.REPEATS))
    for name in kinds:
        say("   %-32s %6.2f [%6.2f, %6.2f]   (worst status of the last step: %d; its mean solver iterations: %.2f; lane changes: %d)"
            % ((name,) + med(res[name]) + last[name][-1]))
    none, follower, lanes = (med(res[name])[0] for name in kinds)
    say("   ratio of the medians: follower= / none %.3f, lanes= / none %.3f, lanes= / follower= %.3f" % (follower / none, lanes / none, lanes / follower))


def main():
    say(T.header())
    say("1. per call, us (median [min, max] of %d repeats; device events around back-to-back calls through the Python host)" % T.REPEATS)
    kernels(4096, 200)
    kernels(32768, 50)
    kernels(262144, 5)
    loops()
    T.finish(sys.argv)


if __name__ == "__main__":
    main()
