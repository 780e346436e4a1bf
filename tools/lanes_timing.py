"""Timing of the lane stage on one MI355X (-> profiles/lanes_timing.txt).

  1. kmpc_lane_step_fleet next to kmpc_follow_fleet and kmpc_waypoints_fleet of the same build at B = 4096, 32768 and 262144: tools/follow_timing.py's
     dense fleet (the three fixture paths, ids interleaved, random poses) on four lanes, the lanes random, a tenth of the vehicles in mid-change; device
     events around REPS back-to-back calls through the Python host, so launch overhead is in.  The stage is timed as the kernel alone (arclengths and
     cross-track errors given; occupancy ping-ponged, the record running) and as Lanes.step() (the geometry-only score call, the on-the-road mask
     and the kernel).  To see where the time goes the kernel is also timed on ONE lane (the four side searches find no band to test, the scan still
     reads every candidate) -- the difference to kmpc_follow_fleet is then the wider tile and the five-fold compare-and-select, not the winners.
  2. kmpc_ref_offset_batch (Lanes.shift on a [B,9,3] table, every offset non-zero) next to the waypoint call.
  3. vehicle-steps per second of ONE ClosedLoop of 4096 vehicles without a stage, with follower= and with lanes= (two lanes): follow_timing's 512
     platoons of eight, so that all three solve the same problems.
Method of tools/fleet_paths_timing.py: the configurations of a group alternate inside one process, five repeats each, median
and range.

usage: python tools/lanes_timing.py [out.txt]
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
    tw, tf, t4, t1, ts, to = [], [], [], [], [], []
    for _ in range(REPEATS):   # alternating
        tw.append(event_time(lambda: fleet.get_waypoints_batch(pose, vt), reps))
        tf.append(event_time(follow_alone, reps))
        t4.append(event_time(lanes_alone(la4), reps))
        t1.append(event_time(lanes_alone(la1), reps))
        ts.append(event_time(lambda: la4.step(st, vt, 2, 0.1, out=out), reps))
        to.append(event_time(lambda: la4.shift(ref), reps))
    say("   B = %d (four lanes: %d vehicles with an own-lane leader; left-ahead %d, left-behind %d, right-ahead %d, right-behind %d), %d calls per repeat:"
        % ((B,) + tuple(found) + (reps,)))
    say("     kmpc_waypoints_fleet, target-velocity mode:                  %10.1f [%10.1f, %10.1f]" % med(tw))
    say("     kmpc_follow_fleet alone (arclengths given):                  %10.1f [%10.1f, %10.1f]" % med(tf))
    say("     kmpc_lane_step_fleet alone, four lanes:                      %10.1f [%10.1f, %10.1f]   %.3f x kmpc_follow_fleet; %.4f ns per follower-candidate pair"
        % (med(t4) + (med(t4)[0] / med(tf)[0], med(t4)[0] * 1e3 / (float(B) * B))))
    say("     kmpc_lane_step_fleet alone, one lane:                        %10.1f [%10.1f, %10.1f]   %.3f x kmpc_follow_fleet" % (med(t1) + (med(t1)[0] / med(tf)[0],)))
    say("     Lanes.step(): score call + on-the-road mask + the kernel:    %10.1f [%10.1f, %10.1f]   %.3f x the waypoint call" % (med(ts) + (med(ts)[0] / med(tw)[0],)))
    say("     kmpc_ref_offset_batch on [B,9,3] (Lanes.shift):              %10.1f [%10.1f, %10.1f]   %.3f x the waypoint call" % (med(to) + (med(to)[0] / med(tw)[0],)))


def loop_rate(B, kind, steps):
    fleet, state = FT.setup(B, B // FT.PLATOON)
    sim = VehicleSimulator(B, X0=state[:, 0], Y0=state[:, 1], Psi0=state[:, 2])
    sim.state[:, 3] = 6.0
    kw = {}
    if kind == "follower":
        kw["follower"] = Follower(fleet)
    elif kind == "lanes":
        kw["lanes"] = Lanes(fleet, lane_rows=lane_params(B, n_lanes=2))
    loop = ClosedLoop(fleet, sim, N=N, target_vel=6.0, **kw)
    for _w in range(20):
        loop.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _s in range(steps):
        o = loop.step()
    torch.cuda.synchronize()
    rate = B * steps / (time.perf_counter() - t0) / 1e6
    changes = int(loop.lanes.summary()["n_changes"].sum()) if kind == "lanes" else 0
    return rate, int(o["status"].max().item()), float(o["iters"].double().mean().item()), changes


def loops(B=4096, steps=100):
    kinds = [("without a stage", None), ("with follower= (default rows)", "follower"), ("with lanes= (two lanes)", "lanes")]
    res, last = {k: [] for k, _ in kinds}, {}
    for _ in range(REPEATS):
        for name, kind in kinds:
            r = loop_rate(B, kind, steps)
            res[name].append(r[0])
            last[name] = r[1:]
    say("2. ClosedLoop of %d vehicles in %d platoons of %d, %g m apart at 6 m/s, N = %d, %d steps per repeat after 20 warm-up steps: M vehicle-steps/s "
        "(median [min, max] of %d, the three loops alternating)" % (B, B // FT.PLATOON, FT.PLATOON, FT.SPACING, N, steps, REPEATS))
    for name, _ in kinds:
        say("   %-32s %6.2f [%6.2f, %6.2f]   (worst status of the last step: %d; its mean solver iterations: %.2f; lane changes: %d)"
            % ((name,) + med(res[name]) + last[name]))
    base = med(res[kinds[0][0]])[0]
    say("   ratio of the medians: follower= / none %.3f, lanes= / none %.3f, lanes= / follower= %.3f"
        % (med(res[kinds[1][0]])[0] / base, med(res[kinds[2][0]])[0] / base, med(res[kinds[2][0]])[0] / med(res[kinds[1][0]])[0]))


def main():
    say("%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    say("1. per call, us (median [min, max] of %d repeats; device events around back-to-back calls through the Python host)" % REPEATS)
    kernels(4096, 200)
    kernels(32768, 50)
    kernels(262144, 5)
    loops()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(FT.LINES) + "\n")


if __name__ == "__main__":
    main()
