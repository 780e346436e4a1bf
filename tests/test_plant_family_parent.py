"""The pedal-driven plant and the measurement stage with faults against tests/golden/plant_family_parent.npz, recorded by
tools/record_stage_golden.py (record-family) on the build before the per-vehicle-row plant kernels were given one body, the five plant kernels one
set of row and state helpers and the measurement kernels one truth-ring fetch: the same raw 64-bit patterns, NaNs compared as bits, no tolerance.
tests/golden/stage_kernels_parent.npz (tests/test_stage_parent.py) predates both stages; together the two files pin the shared bodies.
tests/stage_cases.py holds the cases."""
import os

import numpy as np
import pytest

import stage_cases as SC

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plant_family_parent.npz"))
EVENTS = ("lost_and_regained_gps", "lost_and_regained_imu", "lost_and_regained_spd", "window", "outlier", "blind", "reset", "chain_by_the_draw")


def same(key, got, row=None):
    want = GOLD[key] if row is None else GOLD[key][row]
    assert got.dtype == want.dtype and got.shape == want.shape, key
    if got.tobytes() != want.tobytes():
        a, b = got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)
        rows = np.flatnonzero((a.view(np.uint8).reshape(a.shape[0], -1) != b.view(np.uint8).reshape(b.shape[0], -1)).any(1))
        raise AssertionError("%s: bits differ from the parent build's in rows (lanes of a digest) %s" % (key, rows.tolist()))


@pytest.mark.gpu
@pytest.mark.parametrize("row", range(len(SC.drive_runs())), ids=[r[0] for r in SC.drive_runs()])
def test_drive_kernel(row):
    _name, n, outliers, road, stat = SC.drive_runs()[row]
    hin, h = SC.run_drive(n, outliers, road, stat)
    same("in_drive", hin, slice(row, row + 1))
    same("drive", h, row)


@pytest.mark.gpu
@pytest.mark.parametrize("ring", [False, True], ids=["noring", "ring"])
def test_fault_kernel(ring):
    k = "faults_ring" if ring else "faults"
    ev = SC.fault_events(GOLD["flags_" + k])          # the recorded run did show every event the rows are there for
    assert sorted(ev) == sorted(EVENTS) and all(ev.values()), ev
    hin, h, flags = SC.run_faults(ring)
    same("in_" + k, hin)
    same("flags_" + k, flags)
    same(k, h)


@pytest.mark.parametrize("ring", [False, True], ids=["noring", "ring"])
def test_fault_rows_produce_every_event_on_the_cpu(ring):
    """tests/sensor_fault_ref.py over the same rows: a lost and regained source of each kind, a window, an outlier, a blind vehicle, a record that
    resets; and, the decisions being comparisons of exactly representable numbers, the flags the parent build recorded"""
    flags = SC.fault_flags_cpu(ring)
    ev = SC.fault_events(flags)
    assert sorted(ev) == sorted(EVENTS) and all(ev.values()), ev
    assert np.array_equal(flags, GOLD["flags_faults_ring" if ring else "flags_faults"])
