"""The closed loops' stage kernels and both loops against tests/golden/stage_kernels_parent.npz, recorded by tools/record_stage_golden.py on the build
before the plant kernels were given one sub-step, the stage kernels one set of scalar helpers, the two predict-ahead kernels one loop and the two
loops one period: the same raw 64-bit patterns, NaNs compared as bits, no tolerance.  The "bit for bit" chain tests (default rows = fixed kernel,
queue = plant, neutral road = queue) compare kernels that now share a body; this file is what pins that body.  tests/stage_cases.py holds the cases."""
import os

import numpy as np
import pytest

import stage_cases as SC

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage_kernels_parent.npz"))


def same(key, got, row=None):
    want = GOLD[key] if row is None else GOLD[key][row]
    assert got.dtype == want.dtype and got.shape == want.shape, key
    if got.tobytes() != want.tobytes():
        a, b = got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)
        rows = np.flatnonzero((a.view(np.uint8).reshape(a.shape[0], -1) != b.view(np.uint8).reshape(b.shape[0], -1)).any(1))
        raise AssertionError("%s: bits differ from the parent build's in rows (lanes of a digest) %s" % (key, rows.tolist()))


@pytest.mark.parametrize("row", range(len(SC.plant_runs())), ids=[r[0] for r in SC.plant_runs()])
def test_plant_kernels(row):
    _name, entry, n, outliers, road, stat = SC.plant_runs()[row]
    hin, h = SC.run_plant(entry, n, outliers, road, stat)
    same("in_plant", hin, slice(row, row + 1))
    same("plant", h, row)


@pytest.mark.parametrize("delayed", [False, True])
def test_measurement_kernels(delayed):
    k = "sense_delayed" if delayed else "sense"
    hin, h = SC.run_sense(delayed)
    same("in_" + k, hin)
    same(k, h)


@pytest.mark.parametrize("case", SC.LAT_CASES, ids=lambda c: c[0])
def test_command_in_force_and_both_predictions(case):
    name, first, n = case
    hin, hu, hp, hd = SC.run_latency(first, n)
    same("in_latency_" + name, hin)
    same("cmd_in_force_" + name, hu)
    same("predict_" + name, hp)
    same("predict_dist_" + name, hd)


def test_estimator_observer_and_command_offset():
    hin, he, ho, hc = SC.run_filters()
    same("in_filters", hin)
    same("estimate", he)
    same("observe", ho)
    same("cmd_offset", hc)


@pytest.mark.parametrize("kind", ["cartesian", "frenet"])
def test_closed_loops_with_every_stage_on(kind):
    st = GOLD["loop_starts"]
    out = SC.run_loop(kind, st[0], st[1], st[2])
    assert GOLD["loop_%s_sat" % kind][:, 0:2].sum() > 0      # the road did saturate in the recorded run
    for k in SC.LOOP_KEYS + ("sat",):
        same("loop_%s_%s" % (kind, k), out[k])
