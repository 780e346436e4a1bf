"""Timing of the range sensor and leader tracker on one MI355X (-> profiles/range_timing.txt).

  1. kmpc_range_follow_batch next to kmpc_wander_batch and kmpc_follow_fleet of the same build at B = 4096, 32768 and 262144: the default radar row
     (noise on, FILTER = 1) behind tools/follow_timing.py's dense fleet on the three fixture paths, so that nearly every vehicle detects, predicts
     and updates; device events around REPS back-to-back calls through the Python host, so launch overhead is in.  The kernel moves the sensor row
     (11 words read), the follow row (4), the record (16 read, 16 written), truth, leader, two speeds, cap, cap out and meas: about 0.45 KB per
     vehicle and call.
  2. vehicle-steps per second of ONE ClosedLoop of 4096 vehicles with follower= without and with radar=: tools/follow_timing.py's 512 platoons of
     eight, alternating runs.
Method of tools/fleet_paths_timing.py: the configurations of a group alternate inside one process, five repeats each, median
and range.

usage: python tools/range_timing.py [out.txt]
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
from mkz_mpc_path_follower_amd.ref_traj import Follower, RangeSensor  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator, Wander, wander_rows  # noqa: E402

REPEATS = FT.REPEATS
say, med, event_time = FT.say, FT.med, FT.event_time
BYTES = 8 * (11 + 4 + 16 + 16 + 2 + 2 + 1 + 1 + 4) + 4     # per vehicle and call


def kernels(B, reps):
    rng = np.random.default_rng(1)
    paths = [FT.path_dict(f) for f in FT.FILES]
    pid = np.arange(B) % 3
    fleet = FleetRefTrajectory(paths, pid, traj_horizon=FT.N)
    state = np.zeros((B, 8))
    for p, tr in enumerate(fleet.trajectories):
        sel = np.where(pid == p)[0]
        idx = rng.integers(0, int(0.6 * len(tr)), len(sel))
        state[sel, 0], state[sel, 1], state[sel, 2] = tr[idx, 4] + rng.uniform(-1, 1, len(sel)), tr[idx, 5] + rng.uniform(-1, 1, len(sel)), tr[idx, 3]
    state[:, 3] = rng.uniform(2.0, 8.0, B)
    st = torch.as_tensor(state, device="cuda")
    vt = torch.full((B,), 6.0, dtype=torch.float64, device="cuda")
    dev = torch.device("cuda", 0)
    radar = RangeSensor(B, seed=5)
    fo = Follower(fleet, radar=radar)
    out = torch.empty((B,), dtype=torch.float64, device="cuda")
    fo.cap(st, vt, out=out, k=0, dt=0.1)
    torch.cuda.synchronize()
    err = fo._track["err"]
    L = fleet._lib
    period = [1]

    def range_alone():
        L.kmpc_range_follow_batch(0, B, 0.1, ptr(fo.gap_leader), ptr(fo.leader), ptr(st[:, 3]), 8, ptr(st[:, 3]), 8, ptr(fo.rows), ptr(radar.rows),
                                  radar.seed, period[0], 0, ptr(vt), ptr(out), ptr(radar.rec), ptr(radar.meas), stream(dev))
        period[0] += 1

    def follow_alone():
        L.kmpc_follow_fleet(0, B, ptr(err[:, 3]), 4, ptr(st[:, 3]), 8, ptr(fleet.path_id), None, ptr(fo.rows), ptr(vt), ptr(fo.v_ideal),
                            ptr(fo.gap_leader), ptr(fo.leader), ptr(fo.stat), stream(dev))
    wander = Wander(B, wander_rows(B, sigma=(0.2, 0.2, 0.01, 0.1, 0.3, 0.3, 0.01, 0.1), tau=5.0), seed=3)
    sensor_base = torch.zeros((B, 8), dtype=torch.float64, device="cuda")
    sensor_out, road_base, road_out = torch.zeros_like(sensor_base), torch.zeros_like(sensor_base), torch.zeros_like(sensor_base)
    tr_, tf, tw = [], [], []
    for _ in range(REPEATS):   # alternating
        tr_.append(event_time(range_alone, reps))
        tf.append(event_time(follow_alone, reps))
        tw.append(event_time(lambda: wander.step(period[0], sensor_base, sensor_out, road_base, road_out), reps))
    s = radar.summary()
    say("   B = %d (%d of the last call's vehicles with a track), %d calls per repeat:" % (B, int((s["track_id"] >= 0).sum()), reps))
    say("     kmpc_range_follow_batch (default row: noise, FILTER = 1):   %10.1f [%10.1f, %10.1f]   %.2f ns and %d B per vehicle: %.0f GB/s"
        % (med(tr_) + (med(tr_)[0] * 1e3 / B, BYTES, BYTES * B / med(tr_)[0] / 1e3)))
    say("     kmpc_wander_batch (eight channels on, both row pairs):       %10.1f [%10.1f, %10.1f]   the range stage is %.3f x this"
        % (med(tw) + (med(tr_)[0] / med(tw)[0],)))
    say("     kmpc_follow_fleet alone (arclengths given):                  %10.1f [%10.1f, %10.1f]   the range stage is %.4f x this"
        % (med(tf) + (med(tr_)[0] / med(tf)[0],)))


def loop_rate(B, with_radar, steps):
    fleet, state = FT.setup(B, B // FT.PLATOON)
    sim = VehicleSimulator(B, X0=state[:, 0], Y0=state[:, 1], Psi0=state[:, 2])
    sim.state[:, 3] = 6.0
    loop = ClosedLoop(fleet, sim, N=FT.N, target_vel=6.0, follower=Follower(fleet, radar=RangeSensor(B, seed=5) if with_radar else None))
    for _w in range(20):
        loop.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _s in range(steps):
        o = loop.step()
    torch.cuda.synchronize()
    rate = B * steps / (time.perf_counter() - t0) / 1e6
    return rate, int(o["status"].max().item()), float(o["iters"].double().mean().item()), int(loop.follower.summary()["n_contact"].sum())


def loops(B=4096, steps=100):
    kinds = [("follower= without radar=", False), ("follower= with radar= (default row)", True)]
    res = {k: [] for k, _ in kinds}
    last = {}
    for _ in range(REPEATS):
        for name, wr in kinds:
            r = loop_rate(B, wr, steps)
            res[name].append(r[0])
            last[name] = r[1:]
    say("2. ClosedLoop of %d vehicles in %d platoons of %d, %g m apart at 6 m/s, N = %d, %d steps per repeat after 20 warm-up steps: M vehicle-steps/s "
        "(median [min, max] of %d)" % (B, B // FT.PLATOON, FT.PLATOON, FT.SPACING, FT.N, steps, REPEATS))
    for name, _ in kinds:
        say("   %-38s %6.2f [%6.2f, %6.2f]   (worst status of the last step: %d; its mean solver iterations: %.2f; vehicle-periods in contact: %d)"
            % ((name,) + med(res[name]) + last[name]))
    say("   ratio of the medians with / without: %.3f" % (med(res[kinds[1][0]])[0] / med(res[kinds[0][0]])[0]))


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
