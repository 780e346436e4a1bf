"""Timing of car following on one MI355X (-> profiles/follow_timing.txt).

  1. kmpc_follow_fleet next to kmpc_waypoints_fleet of the same build at B = 4096, 32768 and 262144 on the three fixture paths
     (tests/golden/path{1,2,3}_decimated.npz), path ids interleaved, random poses: a dense fleet, nearly every vehicle has a leader; the calls go
     through the Python host, so launch overhead is in.  The stage is timed as the kernel alone (arclengths given) and as
     Follower.cap() (the geometry-only kmpc_track_score_fleet call, the on-the-road mask and the kernel); the score call is timed separately.
     The pair search is B^2 comparisons whatever the paths are: the number of paths changes how many candidates match, not how many are read.
  2. vehicle-steps per second of ONE ClosedLoop of 4096 vehicles without and with follower=: 512 platoons of eight, 20 m apart at 6 m/s, each on
     its own copy of a fixture path, so that the cap rarely binds and both loops solve the same problems.
  `python tools/follow_timing.py plain` prints the rate of the loop without follower= alone, five repeats: run alternately on this build and on
  the parent commit's (KMPC_TREE=<its checkout>), it shows that a loop without the stage costs what it cost.
Method: tools/_timing.py.

usage: python tools/follow_timing.py [plain | out.txt]
"""
import sys

import numpy as np
import torch

import _timing as T
from _timing import med, say
from mkz_mpc_path_follower_amd._stage import ptr, stream  # noqa: E402
from mkz_mpc_path_follower_amd.ref_traj import Follower  # noqa: E402

N, PLATOON = T.N, T.PLATOON


def kernels(B, reps):
    fleet, state = T.dense_fleet(B, np.random.default_rng(1))
    st = torch.as_tensor(state, device="cuda")
    pose = st[:, 0:3].contiguous()
    vt = torch.full((B,), 6.0, dtype=torch.float64, device="cuda")
    fo = Follower(fleet)
    out = torch.empty((B,), dtype=torch.float64, device="cuda")
    fo.cap(st, vt, out=out)
    torch.cuda.synchronize()
    with_leader = int((fo.leader >= 0).sum().item())
    err, dev = fo._track["err"], torch.device("cuda", 0)
    track = dict(fo._track)

    def kernel_alone():
        fleet._lib.kmpc_follow_fleet(0, B, ptr(err[:, 3]), 4, ptr(st[:, 3]), 8, ptr(fleet.path_id), None, ptr(fo.rows), ptr(vt), ptr(out),
                                     ptr(fo.gap_leader), ptr(fo.leader), ptr(fo.stat), stream(dev))
    t = T.rotate({"waypoints": (lambda: fleet.get_waypoints_batch(pose, vt), reps), "kernel": (kernel_alone, reps),
                  "score": (lambda: fleet.track_score_batch(st, score=None, out=track), reps), "cap": (lambda: fo.cap(st, vt, out=out), reps)})
    tw, tk, ts, tc = med(t["waypoints"]), med(t["kernel"]), med(t["score"]), med(t["cap"])
    say("   B = %d (%d vehicles with a leader), %d calls per repeat:" % (B, with_leader, reps))
    say("     kmpc_waypoints_fleet, target-velocity mode:                  %10.1f [%10.1f, %10.1f]" % tw)
    say("     kmpc_follow_fleet alone (arclengths given):                  %10.1f [%10.1f, %10.1f]   %.3f x the waypoint call; %.4f ns per follower-candidate pair"
        % (tk + (tk[0] / tw[0], tk[0] * 1e3 / (float(B) * B))))
    say("     kmpc_track_score_fleet, geometry only (score = None):        %10.1f [%10.1f, %10.1f]" % ts)
    say("     Follower.cap(): score call + on-the-road mask + the kernel:  %10.1f [%10.1f, %10.1f]   %.3f x the waypoint call" % (tc + (tc[0] / tw[0],)))


def make_loop(B, with_follower):
    fleet, state = T.platoons(B, B // PLATOON)
    return T.platoon_loop(fleet, state, **(dict(follower=Follower(fleet)) if with_follower else {}))


def last_step(loop, o):
    bound = int(loop.follower.summary()["n_bound"].sum()) if loop.follower is not None else 0
    return int(o["status"].max().item()), float(o["iters"].double().mean().item()), bound


def loops(B=4096, steps=100):
    kinds = {"without follower=": False, "with follower= (default rows)": True}
    res, last = T.loop_rates(list(kinds), lambda k: make_loop(B, kinds[k]), B, steps, advance=T.step_periods, after=last_step)
    say("2. ClosedLoop of %d vehicles in %d platoons of %d, %g m apart at 6 m/s, N = %d, %d steps per repeat after 20 warm-up steps: M vehicle-steps/s "
        "(median [min, max] of %d)" % (B, B // PLATOON, PLATOON, T.SPACING, N, steps, T.REPEATS))
    for name in kinds:
        say("   %-32s %6.2f [%6.2f, %6.2f]   (worst status of the last step: %d; its mean solver iterations: %.2f; vehicle-periods in which the cap bound: %d)"
            % ((name,) + med(res[name]) + last[name][-1]))
    without, with_ = kinds
    say("   ratio of the medians with / without: %.3f" % (med(res[with_])[0] / med(res[without])[0]))


def plain(B=4096, steps=100):
    rates = T.loop_rates(["plain"], lambda k: make_loop(B, False), B, steps, advance=T.step_periods)[0]["plain"]
    print("loop without follower=, %d vehicles, tree %s: M vehicle-steps/s %s, median %.2f" % (B, T.ROOT, " ".join("%.2f" % r for r in rates), med(rates)[0]),
          flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "plain":
        return plain()
    say(T.header())
    say("1. per call, us (median [min, max] of %d repeats; device events around back-to-back calls through the Python host)" % T.REPEATS)
    kernels(4096, 200)
    kernels(32768, 50)
    kernels(262144, 5)
    loops()
    T.finish(sys.argv)


if __name__ == "__main__":
    main()
