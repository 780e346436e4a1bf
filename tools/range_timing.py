"""Timing of the range sensor and leader tracker on one MI355X (-> profiles/range_timing.txt).

  1. kmpc_range_follow_batch next to kmpc_wander_batch and kmpc_follow_fleet of the same build at B = 4096, 32768 and 262144: the default radar row
     (noise on, FILTER = 1) behind the dense fleet of tools/_timing.py on the three fixture paths, so that nearly every vehicle detects, predicts
     and updates; the calls go through the Python host, so launch overhead is in.  The kernel moves the sensor row
     (11 words read), the follow row (4), the record (16 read, 16 written), truth, leader, two speeds, cap, cap out and meas: about 0.45 KB per
     vehicle and call.
  2. vehicle-steps per second of ONE ClosedLoop of 4096 vehicles with follower= without and with radar=: the 512 platoons of eight of
     tools/_timing.py, alternating runs.
Method: tools/_timing.py.

usage: python tools/range_timing.py [out.txt]
"""
import sys

import numpy as np
import torch

import _timing as T
from _timing import med, say
from mkz_mpc_path_follower_amd._stage import ptr, stream  # noqa: E402
from mkz_mpc_path_follower_amd.ref_traj import Follower, RangeSensor  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import Wander, wander_rows  # noqa: E402

BYTES = 8 * (11 + 4 + 16 + 16 + 2 + 2 + 1 + 1 + 4) + 4     # per vehicle and call


def kernels(B, reps):
    fleet, state = T.dense_fleet(B, np.random.default_rng(1))
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
    t = T.rotate({"range": (range_alone, reps), "follow": (follow_alone, reps),
                  "wander": (lambda: wander.step(period[0], sensor_base, sensor_out, road_base, road_out), reps)})
    tr_, tf, tw = med(t["range"]), med(t["follow"]), med(t["wander"])
    s = radar.summary()
    say("   B = %d (%d of the last call's vehicles with a track), %d calls per repeat:" % (B, int((s["track_id"] >= 0).sum()), reps))
    say("     kmpc_range_follow_batch (default row: noise, FILTER = 1):   %10.1f [%10.1f, %10.1f]   %.2f ns and %d B per vehicle: %.0f GB/s"
        % (tr_ + (tr_[0] * 1e3 / B, BYTES, BYTES * B / tr_[0] / 1e3)))
    say("     kmpc_wander_batch (eight channels on, both row pairs):       %10.1f [%10.1f, %10.1f]   the range stage is %.3f x this"
        % (tw + (tr_[0] / tw[0],)))
    say("     kmpc_follow_fleet alone (arclengths given):                  %10.1f [%10.1f, %10.1f]   the range stage is %.4f x this"
        % (tf + (tr_[0] / tf[0],)))


def make_loop(B, with_radar):
    fleet, state = T.platoons(B, B // T.PLATOON)
    return T.platoon_loop(fleet, state, follower=Follower(fleet, radar=RangeSensor(B, seed=5) if with_radar else None))


def last_step(loop, o):
    return int(o["status"].max().item()), float(o["iters"].double().mean().item()), int(loop.follower.summary()["n_contact"].sum())


def loops(B=4096, steps=100):
    kinds = {"follower= without radar=": False, "follower= with radar= (default row)": True}
    res, last = T.loop_rates(list(kinds), lambda k: make_loop(B, kinds[k]), B, steps, advance=T.step_periods, after=last_step)
    say("2. ClosedLoop of %d vehicles in %d platoons of %d, %g m apart at 6 m/s, N = %d, %d steps per repeat after 20 warm-up steps: M vehicle-steps/s "
        "(median [min, max] of %d)" % (B, B // T.PLATOON, T.PLATOON, T.SPACING, T.N, steps, T.REPEATS))
    for name in kinds:
        say("   %-38s %6.2f [%6.2f, %6.2f]   (worst status of the last step: %d; its mean solver iterations: %.2f; vehicle-periods in contact: %d)"
            % ((name,) + med(res[name]) + last[name][-1]))
    without, with_ = kinds
    say("   ratio of the medians with / without: %.3f" % (med(res[with_])[0] / med(res[without])[0]))


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
