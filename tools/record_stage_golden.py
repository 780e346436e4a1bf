"""Records tests/golden/stage_kernels_parent.npz (tests/test_stage_parent.py): what the closed loops' stage kernels -- the four plant kernels, the two
measurement kernels, command-in-force and the two predict-ahead kernels, estimator, observer and command offset -- and both closed loops with every
stage on compute on the build that is loaded, as bit patterns; and tests/golden/plant_family_parent.npz (tests/test_plant_family_parent.py): the
same for the pedal-driven plant and the measurement stage with faults.  Run it from the commit whose outputs a later change has to reproduce,
before that change (KMPC_LIB names another build of the library, as for the other tools).

  python tools/record_stage_golden.py record [OUT.npz]
  python tools/record_stage_golden.py check [IN.npz]     replay against the file and list the keys that differ
  python tools/record_stage_golden.py record-family [OUT.npz]      the second file
  python tools/record_stage_golden.py check-family [IN.npz]

tests/stage_cases.py holds the cases, their inputs and what a key of the file means."""
import os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def replay(starts=None):
    """every case on the loaded build -> dict key -> array, as the file holds them"""
    import stage_cases as SC
    out = {}
    runs = [SC.run_plant(entry, n, outliers, road, stat) for _name, entry, n, outliers, road, stat in SC.plant_runs()]
    out["in_plant"], out["plant"] = np.concatenate([r[0] for r in runs]), np.stack([r[1] for r in runs])   # rows in plant_runs()'s order
    for delayed in (False, True):
        k = "sense_delayed" if delayed else "sense"
        out["in_" + k], out[k] = SC.run_sense(delayed)
    for name, first, n in SC.LAT_CASES:
        out["in_latency_" + name], out["cmd_in_force_" + name], out["predict_" + name], out["predict_dist_" + name] = SC.run_latency(first, n)
    out["in_filters"], out["estimate"], out["observe"], out["cmd_offset"] = SC.run_filters()
    if starts is None:   # the loops' starts come from the CPU oracle's trajectory table (sin / cos of the host): the file carries them
        import latency_ref as LR
        starts = np.stack(LR.starts(SC.LOOP_NV)[0:3])
    out["loop_starts"] = starts
    for kind in ("cartesian", "frenet"):
        for k, v in SC.run_loop(kind, starts[0], starts[1], starts[2]).items():
            out["loop_%s_%s" % (kind, k)] = v
    return out


def replay_family(_starts=None):
    """the second file's cases on the loaded build"""
    import stage_cases as SC
    out = {}
    runs = [SC.run_drive(n, outliers, road, stat) for _name, n, outliers, road, stat in SC.drive_runs()]
    out["in_drive"], out["drive"] = np.concatenate([r[0] for r in runs]), np.stack([r[1] for r in runs])   # rows in drive_runs()'s order
    for ring in (False, True):
        k = "faults_ring" if ring else "faults"
        out["in_" + k], out[k], out["flags_" + k] = SC.run_faults(ring)
    return out


def main(argv):
    if len(argv) < 2 or argv[1] not in ("record", "check", "record-family", "check-family"):
        sys.exit(__doc__)
    family = argv[1].endswith("-family")
    default = os.path.join(ROOT, "tests", "golden", "plant_family_parent.npz" if family else "stage_kernels_parent.npz")
    run = replay_family if family else replay
    path = argv[2] if len(argv) > 2 else default
    if os.environ.get("KMPC_LIB"):
        from mkz_mpc_path_follower_amd import _lib
        _lib.LIB_PATH = os.path.abspath(os.environ["KMPC_LIB"])
    if argv[1].startswith("record"):
        out = run()
        np.savez_compressed(path, **out)
        print("wrote %s: %d keys, %d bytes" % (path, len(out), os.path.getsize(path)))
        return 0
    gold = np.load(path)
    out = run(None if family else gold["loop_starts"])
    bad = [k for k in gold.files if out[k].dtype != gold[k].dtype or out[k].tobytes() != gold[k].tobytes()]
    print("%d of %d keys differ%s" % (len(bad), len(gold.files), ": " + ", ".join(bad) if bad else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
