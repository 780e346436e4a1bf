"""Timing of the pedal-driven plant (kmpc_sim_advance_drive) next to the road plant it extends, on one MI355X (-> profiles/drive_timing.txt).

One control period (10 updates = 100 sub-steps and 5 ticks of the low-level controller, depth 2, no delay, neutral road rows, default drive and
controller rows, with road_stat) of
  - kmpc_sim_advance_road of the PARENT build: a libkmpc_hip.so built from the commit before this kernel existed, given as --parent-lib (without it
    this build's kmpc_sim_advance_road stands in, and the output says so; tools/isa_diff.py shows its instructions are the parent's);
  - kmpc_sim_advance_road of this build;
  - kmpc_sim_advance_drive;
  - kmpc_llc_step_batch alone, five ticks (what the node costs as a stage of its own)
at B = 4096 and B = 262 144; every variant restarts from the same states in every repeat.  Method: tools/_timing.py.
No target is set: the tick is a few dozen operations per 20 sub-steps, and the sub-step gains two lags and one multiply-add chain.

usage: python tools/drive_timing.py [--parent-lib PATH/libkmpc_hip.so] [out.txt]
"""
import ctypes as C
import sys

import numpy as np
import torch

import _timing as T
from _timing import med, say
from mkz_mpc_path_follower_amd import _lib  # noqa: E402
from mkz_mpc_path_follower_amd.vehicle_sim import drive_params, llc_params, plant_params, road_params  # noqa: E402

REPS = 100


def main():
    args = sys.argv[1:]
    parent = None
    if "--parent-lib" in args:
        i = args.index("--parent-lib")
        parent = args[i + 1]
        del args[i:i + 2]
    L = _lib.load()
    LP = L
    if parent is not None:
        LP = C.CDLL(parent)
        LP.kmpc_sim_advance_road.argtypes = L.kmpc_sim_advance_road.argtypes
        assert not hasattr(LP, "kmpc_sim_advance_drive"), "the parent build has no pedal-driven plant"
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    say(T.header())
    say("us per control period, median [min, max] of %d repeats of %d back-to-back launches; parent build: %s"
        % (T.REPEATS, REPS, "a separate library built from the parent commit" if parent else "NOT GIVEN, this build's kmpc_sim_advance_road stands in"))
    for B in (4096, 262144):
        rng = np.random.default_rng(B)
        s0 = np.zeros((B, 8))
        s0[:, 0:2] = rng.uniform(-500, 500, (B, 2)); s0[:, 2] = rng.uniform(-np.pi, np.pi, B); s0[:, 3] = rng.uniform(4, 12, B)
        s0[:, 4] = rng.uniform(-0.1, 0.1, B); s0[:, 5] = rng.uniform(-0.1, 0.1, B); s0[:, 7] = rng.uniform(-0.1, 0.1, B)
        rec0 = np.zeros((B, 16))
        rec0[:, 3] = s0[:, 3]                  # V_LAST: the controllers start at speed
        s0, rec0 = torch.as_tensor(s0, device="cuda"), torch.as_tensor(rec0, device="cuda")
        # the command holds the speed and keeps steering: the states stay in the polynomials' ranges over the 103 periods of a repeat
        cmd = torch.as_tensor(np.stack([np.zeros(B), rng.uniform(-0.1, 0.1, B)], 1), device="cuda")
        plant, road, drive, llc = plant_params(B), road_params(B), drive_params(B), llc_params(B)
        names = ("kmpc_sim_advance_road, parent build", "kmpc_sim_advance_road, this build", "kmpc_sim_advance_drive", "kmpc_llc_step_batch x 5")
        st = {k: s0.clone() for k in names}
        qu = {k: cmd.repeat(2, 1, 1).contiguous() for k in names}
        stat = {k: torch.zeros((B, 4), dtype=torch.float64, device="cuda") for k in names}
        rec = {k: rec0.clone() for k in names}
        per = {k: 0 for k in names}

        def road_call(k, lib):
            def fn():
                per[k] += 1
                return lib.kmpc_sim_advance_road(0, B, p(st[k]), p(cmd), p(plant), p(road), None, p(qu[k]), 2, per[k], 10, p(stat[k]), None)
            return fn

        def drive_call():
            k = names[2]
            per[k] += 1
            return L.kmpc_sim_advance_drive(0, B, p(st[k]), p(cmd), p(plant), p(road), p(drive), p(llc), p(rec[k]), None, p(qu[k]), 2, per[k], 10,
                                            p(stat[k]), None)

        def stage_call():
            k = names[3]
            rc = 0
            for _ in range(5):
                rc |= L.kmpc_llc_step_batch(0, B, p(cmd), C.c_void_p(st[k].data_ptr() + 24), 8, p(llc), p(rec[k]), None, None)
            return rc
        run = {names[0]: road_call(names[0], LP), names[1]: road_call(names[1], L), names[2]: drive_call, names[3]: stage_call}
        for k, fn in run.items():
            assert fn() == 0, k
        def restart():
            for k in names:
                st[k].copy_(s0); stat[k].zero_(); rec[k].copy_(rec0)
        res = T.rotate({k: (fn, REPS) for k, fn in run.items()}, before=restart)
        torch.cuda.synchronize()
        assert all(torch.isfinite(t).all().item() for t in st.values()) and torch.isfinite(rec[names[2]]).all().item()
        assert torch.equal(st[names[0]], st[names[1]])
        for k in names:
            say("   B = %-7d %-40s %8.1f [%8.1f, %8.1f]" % ((B, k) + med(res[k])))
        say("   B = %-7d this build's road plant = the parent build's states bit for bit after %d periods; drive / parent road = %.3f"
            % (B, REPS + 3, med(res[names[2]])[0] / med(res[names[0]])[0]))
    T.finish(sys.argv[:1] + args)


if __name__ == "__main__":
    main()
