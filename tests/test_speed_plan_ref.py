"""CPU side of the speed plan (kmpc_pathset_curvature, kmpc_speed_plan_default, kmpc_speed_plan_fleet): the symbols and their argument checks (no
GPU needed: every check comes before the first device call), self-checks of the numpy restatement tests/speed_plan_ref.py, the branch counts of
the committed 300-vehicle draw that tests/test_speed_plan.py runs on the device, and the one-vehicle CPU loop through path3's tight corner with
and without the plan."""
import ctypes as C

import numpy as np
import pytest

import speed_plan_ref as SP

ARG = -1   # KMPC_ERR_ARG


def test_symbols_default_rows_and_abi_version():
    from mkz_mpc_path_follower_amd import _lib
    L = _lib.load()
    for name in ("kmpc_pathset_curvature", "kmpc_speed_plan_default", "kmpc_speed_plan_fleet"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.kmpc_abi_version() == 8
    r = np.full((3, 8), 7.0)
    assert L.kmpc_speed_plan_default(r.ctypes.data_as(C.POINTER(C.c_double)), 3) == 0
    assert r[0].tolist() == [2.0, 0.7, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0] and np.array_equal(r, np.tile(SP.DEFAULT_ROW, (3, 1)))
    assert L.kmpc_speed_plan_default(None, 1) == ARG and b"kmpc_speed_plan_default" in L.kmpc_last_error(None)
    assert L.kmpc_speed_plan_default(r.ctypes.data_as(C.POINTER(C.c_double)), -1) == ARG
    assert L.kmpc_speed_plan_default(None, 0) == 0
    from mkz_mpc_path_follower_amd import ref_traj as RT
    assert np.array_equal(RT.speed_plan_default(), SP.DEFAULT_ROW) and RT.PLAN_FIELDS == SP.FIELDS
    for bad in (dict(a_lat=0.0), dict(a_lat=np.nan), dict(a_brake=0.0), dict(a_brake=np.inf), dict(v_floor=-1.0), dict(v_floor=np.inf),
                dict(end_stop=np.nan)):
        with pytest.raises(ValueError):
            RT.check_speed_plan_rows(SP.rows(2, **bad))
    RT.check_speed_plan_rows(SP.rows(2, a_lat=np.inf, end_stop=1.0))


def test_argument_checks_answer_before_any_device_call():
    from mkz_mpc_path_follower_amd import _lib
    L = _lib.load()
    p = C.c_void_p(64)   # never dereferenced: every call below is refused on the host
    q = dict(ps=p, B=2, kappa=p, state=p, stride=8, pid=p, v_cap=p, rows=p, v_plan=p, info=p, closest=p)

    def plan(**kw):
        a = dict(q, **kw)
        return L.kmpc_speed_plan_fleet(a["ps"], a["B"], a["kappa"], a["state"], a["stride"], a["pid"], a["v_cap"], a["rows"], a["v_plan"], a["info"],
                                       a["closest"], None)
    for bad in (dict(ps=None), dict(B=-1), dict(stride=1), dict(stride=0), dict(kappa=None), dict(state=None), dict(pid=None), dict(v_cap=None),
                dict(rows=None), dict(v_plan=None), dict(ps=None, B=0)):
        assert plan(**bad) == ARG, bad
        assert b"kmpc_speed_plan_fleet" in L.kmpc_last_error(None)
    for bad in ((None, 4.0, p), (p, 0.0, p), (p, -1.0, p), (p, np.nan, p), (p, np.inf, p), (p, 4.0, None)):
        assert L.kmpc_pathset_curvature(bad[0], bad[1], bad[2], None) == ARG, bad
        assert b"kmpc_pathset_curvature" in L.kmpc_last_error(None)


# ---------------------------------------------------------------- the restatement's own properties
def test_unlimited_row_returns_the_cap_itself():
    """A_LAT = inf, END_STOP = 0: v_plan == v_cap exactly, for every vehicle of the draw (the w == vcap2 select, not a sqrt of a square)"""
    d = SP.draw()
    r = SP.rows(SP.DRAW_B, a_lat=np.inf, a_brake=d["rows"][:, 1], v_floor=d["rows"][:, 2])
    o = SP.plan(SP.five_trajectories(), SP.five_kappas(), d["path_id"], d["x"], d["y"], d["v_cap"], r)
    assert not o["refused"].any() and np.array_equal(o["v_plan"], d["v_cap"]) and (o["d_bind"] == 0.0).all()


def test_plan_is_monotone_in_curvature_and_braking():
    """v_plan is non-increasing when |kappa| is scaled up and non-decreasing in A_BRAKE"""
    d = SP.draw()
    trajs, kap = SP.five_trajectories(), SP.five_kappas()
    last = None
    for scale in (0.5, 1.0, 2.0, 4.0):
        o = SP.plan(trajs, [k * scale for k in kap], d["path_id"], d["x"], d["y"], d["v_cap"], d["rows"])
        assert last is None or (o["v_plan"] <= last).all(), scale
        last = o["v_plan"]
    last = None
    for f in (0.5, 1.0, 2.0):
        r = d["rows"].copy()
        r[:, 1] *= f
        o = SP.plan(trajs, kap, d["path_id"], d["x"], d["y"], d["v_cap"], r)
        assert last is None or (o["v_plan"] >= last).all(), f
        last = o["v_plan"]


def test_five_paths_have_no_empty_window_and_a_monotone_arclength():
    """at window 4.0 no sample of fleet_scenario.five_paths() has den == 0, and s is non-decreasing on every path (what the early exit rests on);
    the heading-difference curvature stays below 0.1 1/m on the long paths where three-point curvature reaches 2 1/m"""
    peak = []
    for tr in SP.five_trajectories():
        kap, den = SP.curvature(tr, SP.WINDOW)
        assert (den > 0.0).all() and (np.diff(tr[:, 6]) >= 0.0).all() and np.isfinite(kap).all()
        peak.append(np.fabs(kap).max())
    print("largest |kappa| at window 4 m on the five paths:", np.round(peak, 4))
    assert all(0.05 < peak[p] < 0.1 for p in SP.LONG)


def test_the_committed_draw_exercises_every_branch():
    """branch counts of the 300-vehicle draw (seed 77) on the restatement: limited 104, bound ahead through curvature on a long path 25, binding
    sample more than 64 samples ahead 15, at the floor 30, at a path's last sample 30, bound by END_STOP 63 (printed; the floors asserted are 40, 20,
    5, 10, 10, 10)"""
    d, o = SP.draw(), SP.draw_plan()
    trajs = SP.five_trajectories()
    M = np.array([len(trajs[p]) for p in d["path_id"]])
    longp = np.isin(d["path_id"], SP.LONG)
    limited = o["v_plan"] < d["v_cap"]
    ahead_curv = (o["d_bind"] > 0.0) & longp & (o["jb"] != M - 1)
    beyond = (o["jb"] - o["closest"]) > 64
    floor = limited & (o["v_plan"] == d["rows"][:, 2])
    at_last = o["closest"] == M - 1
    end_bound = (d["rows"][:, 3] != 0.0) & (o["jb"] == M - 1) & limited
    counts = [int(a.sum()) for a in (limited, ahead_curv, beyond, floor, at_last, end_bound)]
    print("draw: limited %d, bound ahead through curvature on a long path %d, beyond one chunk %d, at the floor %d, at a last sample %d, "
          "bound by END_STOP %d" % tuple(counts))
    assert not o["refused"].any()
    assert all(c >= lo for c, lo in zip(counts, (40, 20, 5, 10, 10, 10))), counts


# ---------------------------------------------------------------- the issue's table as a test
@pytest.mark.parametrize("ri", [0, 1, 2])
def test_the_plan_halves_the_corner_error_on_the_cpu(oracle, ri):
    """path3 from sample int(0.50 M), already at 8 m/s, 220 periods through the path's tight corner, on the neutral road, mu = 0.5 and mu = 0.35:
    every solve Optimal, and the planned loop's largest |e_ct| is at most half the plain loop's (the parent's behaviour).
    Measured (printed): neutral 1.573 -> 0.342 m (ratio 0.217), front-saturated sub-steps 0 -> 0, lowest planned speed 4.575 m/s; mu = 0.5
    8.274 -> 1.081 m (0.131), 7721 -> 1583, 5.551 m/s; mu = 0.35 34.368 -> 0.749 m (0.022), 15135 -> 1985, 4.643 m/s.  All from sample 1104
    (no shift needed: no period's nearest-sample margin fell below 1e-6 in any of the six loops)."""
    plain, tr, i0 = SP.cached_loop(oracle, ri, False)
    planned, _, _ = SP.cached_loop(oracle, ri, True)
    e0, e1 = plain["ect"].max(), planned["ect"].max()
    print("road %s from sample %d: largest |e_ct| plain %.3f m, planned %.3f m (ratio %.3f); front-saturated sub-steps %d -> %d; lowest planned speed "
          "%.3f m/s; nearest-sample margin low: plain %s planned %s" % (SP.LOOP_ROADS[ri] or "neutral", i0, e0, e1, e1 / e0, plain["stat"][0],
                                                                     planned["stat"][0], planned["v_plan"].min(), plain["margin_low"], planned["margin_low"]))
    assert (plain["status"] == 0).all() and (planned["status"] == 0).all()
    assert np.isfinite(planned["state"]).all() and planned["v_plan"].min() < SP.VT and (plain["v_plan"] == SP.VT).all()
    assert e1 <= 0.5 * e0
    assert not planned["margin_low"]      # tests/test_speed_plan.py compares this loop with the device's
