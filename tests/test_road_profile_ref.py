"""CPU side of the road profile (kmpc_road_profile_default, kmpc_road_profile_fleet, kmpc_speed_plan_fleet_profile): the symbols and their argument
checks (no GPU needed: every check comes before the first device call), the host validation of a table, self-checks of the numpy restatement
tests/road_profile_ref.py, the branch counts of the committed 300-vehicle draw that tests/test_road_profile.py runs on the device, and the
one-vehicle CPU loops through path3's tight corner with an ice patch in it: no plan, a plan whose map knows nothing, a plan whose map is the truth;
a 4 m/s zone; a stretch of bank and grade."""
import ctypes as C
import os

import numpy as np
import pytest

import road_profile_ref as RP
import road_ref as RR
import speed_plan_ref as SP

ARG = -1   # KMPC_ERR_ARG


# ---------------------------------------------------------------- 1: symbols and arguments
def test_symbols_default_rows_and_abi_version():
    from mkz_mpc_path_follower_amd import _lib
    L = _lib.load()
    for name in ("kmpc_road_profile_default", "kmpc_road_profile_fleet", "kmpc_speed_plan_fleet_profile"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.kmpc_abi_version() == 8
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    r = np.full((3, 8), 7.0)
    assert L.kmpc_road_profile_default(dp(r), 3) == 0
    assert r[0].tolist() == [1.0, 0.0, 0.0, np.inf, 0.0, 0.0, 0.0, 0.0] and np.array_equal(r, np.tile(RP.NEUTRAL_ROW, (3, 1)))
    assert L.kmpc_road_profile_default(None, 1) == ARG and b"kmpc_road_profile_default" in L.kmpc_last_error(None)
    assert L.kmpc_road_profile_default(dp(r), -1) == ARG
    assert L.kmpc_road_profile_default(None, 0) == 0
    from mkz_mpc_path_follower_amd import vehicle_sim as VS
    assert np.array_equal(VS.road_profile_default(), RP.NEUTRAL_ROW) and VS.PROFILE_FIELDS == RP.FIELDS and VS.PROFILE_WORDS == 8
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "kmpc.h")).read()
    for k, name in enumerate(("MU_SCALE", "A_LONG", "A_LAT", "V_LIMIT")):
        assert "KMPC_PROFILE_%s = %d," % (name, k) in hdr
    assert "KMPC_PROFILE_WORDS = 8" in hdr


def test_argument_checks_answer_before_any_device_call():
    from mkz_mpc_path_follower_amd import _lib
    L = _lib.load()
    p, p2 = C.c_void_p(64), C.c_void_p(128)   # never dereferenced: every call below is refused on the host
    q = dict(ps=p, B=2, profile=p, state=p, stride=8, pid=p, base=p, out=p2, closest=p)

    def compose(**kw):
        a = dict(q, **kw)
        return L.kmpc_road_profile_fleet(a["ps"], a["B"], a["profile"], a["state"], a["stride"], a["pid"], a["base"], a["out"], a["closest"], None)
    for bad in (dict(ps=None), dict(B=-1), dict(stride=1), dict(stride=0), dict(profile=None), dict(state=None), dict(pid=None), dict(base=None),
                dict(out=None), dict(out=p), dict(out=p, B=0), dict(ps=None, B=0)):
        assert compose(**bad) == ARG, bad
        assert b"kmpc_road_profile_fleet" in L.kmpc_last_error(None)
    assert compose(out=p) == ARG and b"road_base" in L.kmpc_last_error(None)   # road_out == road_base: says which rule
    q = dict(ps=p, B=2, kappa=p, profile=p, state=p, stride=8, pid=p, v_cap=p, rows=p, v_plan=p, info=p, closest=p)

    def plan(**kw):
        a = dict(q, **kw)
        return L.kmpc_speed_plan_fleet_profile(a["ps"], a["B"], a["kappa"], a["profile"], a["state"], a["stride"], a["pid"], a["v_cap"], a["rows"],
                                               a["v_plan"], a["info"], a["closest"], None)
    for bad in (dict(ps=None), dict(B=-1), dict(stride=1), dict(stride=0), dict(kappa=None), dict(profile=None), dict(state=None), dict(pid=None),
                dict(v_cap=None), dict(rows=None), dict(v_plan=None), dict(ps=None, B=0)):
        assert plan(**bad) == ARG, bad
        assert b"kmpc_speed_plan_fleet_profile" in L.kmpc_last_error(None)


# ---------------------------------------------------------------- 2: host validation
class _Paths:
    """what road_profile_table / road_profile_patch read of a FleetRefTrajectory: its trajectories"""

    def __init__(self, trajs):
        self.trajectories = trajs


def test_check_road_profile_refuses_each_bad_word_by_name():
    from mkz_mpc_path_follower_amd import vehicle_sim as VS
    good = np.tile(RP.NEUTRAL_ROW, (5, 1))
    good[1] = (0.35, -0.5, 1.5, 4.0, 0.0, 0.0, 0.0, 0.0)
    good[2, 3] = 0.0
    assert VS.check_road_profile(good) is not None
    for w, v, name in ((0, 0.0, "mu_scale"), (0, -1.0, "mu_scale"), (0, np.inf, "mu_scale"), (1, np.inf, "a_long"), (1, -np.inf, "a_long"),
                       (2, np.inf, "a_lat"), (3, -1.0, "v_limit"), (3, -np.inf, "v_limit"), (5, np.inf, "only v_limit"), (7, -np.inf, "only v_limit")):
        t = good.copy()
        t[3, w] = v
        with pytest.raises(ValueError, match=name) as e:
            VS.check_road_profile(t)
        assert "[3]" in str(e.value), (w, v, str(e.value))
    for w in range(8):
        t = good.copy()
        t[4, w] = np.nan
        with pytest.raises(ValueError, match="NaN"):
            VS.check_road_profile(t)
    for shape in ((5,), (5, 7), (2, 5, 8)):
        with pytest.raises(ValueError, match=r"\[n,8\]"):
            VS.check_road_profile(np.ones(shape))


def test_road_profile_patch_touches_only_the_named_paths_samples_inside_the_stretch():
    from mkz_mpc_path_follower_amd import vehicle_sim as VS
    trajs = SP.five_trajectories()
    fleet = _Paths(trajs)
    tab = VS.road_profile_table(fleet)
    off = np.concatenate([[0], np.cumsum([len(tr) for tr in trajs])])
    assert tab.shape == (off[-1], 8) and np.array_equal(tab, RP.flat(RP.table(trajs)))
    s = trajs[2][:, 6]
    n = VS.road_profile_patch(tab, fleet, 2, 100.0, 130.0, mu_scale=0.5, v_limit=3.0)
    inside = np.flatnonzero((s >= 100.0) & (s <= 130.0))
    assert n == len(inside) > 50
    exp = RP.table(trajs)
    exp[2][inside, 0], exp[2][inside, 3] = 0.5, 3.0
    assert np.array_equal(tab, RP.flat(exp))
    assert np.array_equal(RP.patch(RP.table(trajs)[2], trajs[2], 100.0, 130.0, mu_scale=0.5), inside)
    assert VS.road_profile_patch(tab, fleet, 1, 1e6, 2e6, a_lat=1.0) == 0 and np.array_equal(tab, RP.flat(exp))
    n = VS.road_profile_patch(tab, fleet, 3, -1.0, 1e9, a_long=-0.5, a_lat=1.5)
    exp[3][:, 1], exp[3][:, 2] = -0.5, 1.5
    assert n == 65 and np.array_equal(tab, RP.flat(exp))
    VS.check_road_profile(tab)
    with pytest.raises(ValueError, match="unknown word"):
        VS.road_profile_patch(tab, fleet, 0, 0.0, 1.0, df_offset=0.1)
    with pytest.raises(ValueError, match="path"):
        VS.road_profile_patch(tab, fleet, 5, 0.0, 1.0, a_lat=0.1)
    with pytest.raises(ValueError):
        VS.road_profile_patch(tab[:-1], fleet, 0, 0.0, 1.0, a_lat=0.1)
    assert np.array_equal(tab, RP.flat(exp))


# ---------------------------------------------------------------- 3: the restatement's identities
def test_neutral_table_restates_the_plan_and_returns_the_base_rows():
    """with the neutral table the restated plan equals speed_plan_ref.plan on speed_plan_ref.draw() in every key, exactly, and the restated compose
    returns the base rows (a -0.0 in A_LONG comes back as +0.0: equal as numbers)"""
    d, e = SP.draw(), SP.draw_plan()
    trajs = SP.five_trajectories()
    o = RP.plan(trajs, SP.five_kappas(), RP.table(trajs), d["path_id"], d["x"], d["y"], d["v_cap"], d["rows"])
    for k in e:
        assert o[k].tobytes() == e[k].tobytes(), k
    assert set(o) == set(e) | {"kind"}
    dd = RP.draw()
    out, closest = RP.compose(trajs, RP.table(trajs), dd["path_id"], dd["x"], dd["y"], dd["road_base"])
    assert np.array_equal(out, dd["road_base"], equal_nan=True) and (closest >= 0).all()
    assert out[:, 4:8].tobytes() == dd["road_base"][:, 4:8].tobytes()
    assert np.signbit(dd["road_base"][5, 2]) and not np.signbit(out[5, 2])


def test_compose_words_and_refusals_of_the_restatement():
    trajs = SP.five_trajectories()
    tab = RP.table(trajs)
    tab[4][:, :4] = (0.5, -0.25, 1.5, 2.0)
    base = RR.rows(4, mu_f=[np.inf, 0.8, 0.8, 0.8], mu_r=0.6, a_long=0.125, a_lat=-1.0, df_offset=0.01, acc_gain=1.1)
    tr = trajs[4]
    out, closest = RP.compose(trajs, tab, np.array([4, 4, 5, 4]), np.array([tr[7, 4], tr[9, 4], tr[9, 4], np.nan]), np.array([tr[7, 5], tr[9, 5], tr[9, 5], 0.0]), base)
    assert closest.tolist() == [7, 9, -1, -1]
    assert out[0].tolist() == [np.inf, 0.3, -0.125, 0.5, 0.01, 1.1, 0.0, 0.0] and out[1].tolist() == [0.4, 0.3, -0.125, 0.5, 0.01, 1.1, 0.0, 0.0]
    assert np.array_equal(out[2:], base[2:])


# ---------------------------------------------------------------- 4: the committed draw
def test_the_committed_draw_exercises_every_branch():
    """branch counts of the 300-vehicle draw (seed 91) on the restatement: bound by a V_LIMIT sample ahead 63, bound by a scaled cornering limit 29,
    binding sample more than 64 samples ahead 23, own sample inside a patch / zone / stretch 133, bound by a V_LIMIT of exactly 0 mid-path 12,
    unlimited 128 (printed; the floors asserted are the issue's 20, 20, 10, 10, 10, 1).  Nobody refused; the compose changes 100+ rows."""
    d, o = RP.draw(), RP.draw_plan()
    trajs, tab = SP.five_trajectories(), d["table"]
    RP_flat = RP.flat(tab)
    from mkz_mpc_path_follower_amd import vehicle_sim as VS
    VS.check_road_profile(RP_flat)
    assert [len(tr) for tr in trajs][1] == 2 and [len(tr) for tr in trajs][3] == 65 and len(d["path_id"]) == RP.DRAW_B == 300
    M = np.array([len(trajs[p]) for p in d["path_id"]])
    at = lambda idx, w: np.array([tab[p][j, w] for p, j in zip(d["path_id"], idx)])
    limit_ahead = (o["kind"] == RP.LIMIT) & (o["jb"] > o["closest"])
    scaled = (o["kind"] == RP.CORNER) & (at(o["jb"], 0) != 1.0)
    beyond = (o["jb"] - o["closest"]) > 64
    own = np.array([(tab[p][i, :4] != RP.NEUTRAL_ROW[:4]).any() for p, i in zip(d["path_id"], o["closest"])])
    zero = (o["kind"] == RP.LIMIT) & (at(o["jb"], 3) == 0.0) & (o["jb"] != M - 1)
    unlimited = o["v_plan"] == d["v_cap"]
    counts = [int(a.sum()) for a in (limit_ahead, scaled, beyond, own, zero, unlimited)]
    print("draw: bound by a V_LIMIT ahead %d, by a scaled cornering limit %d, beyond one chunk %d, own sample in a patch %d, bound by V_LIMIT 0 "
          "mid-path %d, unlimited %d" % tuple(counts))
    assert not o["refused"].any()
    assert all(c >= lo for c, lo in zip(counts, (20, 20, 10, 10, 10, 1))), counts
    out, closest = RP.draw_compose()
    changed = (out[:, :4] != d["road_base"][:, :4]).any(1)
    assert np.array_equal(closest, o["closest"]) and changed.sum() >= 100 and out[:, 4:8].tobytes() == d["road_base"][:, 4:8].tobytes()
    assert np.isnan(d["road_base"][:, 6:8]).any() and np.isinf(d["road_base"][:, 6:8]).any()
    # the map makes a difference: the plan without it differs for the vehicles it binds
    plain = SP.plan(trajs, SP.five_kappas(), d["path_id"], d["x"], d["y"], d["v_cap"], d["rows"])
    assert (plain["v_plan"] >= o["v_plan"]).all() and (plain["v_plan"] > o["v_plan"]).sum() >= 60


# ---------------------------------------------------------------- 5: the issue's table as tests
def test_corner_patch_is_the_issues():
    """MU_SCALE 0.35 on the samples within 10 m of a sample with |kappa| >= 0.03 at window 4 m: 235 samples of path3, s = 314.7 ... 353.2 m
    (printed), one unbroken run"""
    _, _, _, tr, i0 = SP.loop_start()
    prof, idx = RP.corner_patch(tr)
    print("patch: %d samples, s = %.1f ... %.1f m; start sample %d at s = %.1f m" % (len(idx), tr[idx[0], 6], tr[idx[-1], 6], i0, tr[i0, 6]))
    assert len(idx) == 235 and abs(tr[idx[0], 6] - 314.7) < 0.06 and abs(tr[idx[-1], 6] - 353.2) < 0.06
    assert (np.diff(idx) == 1).all() and (prof[idx, 0] == 0.35).all() and np.array_equal(np.delete(prof, idx, 0), np.tile(RP.NEUTRAL_ROW, (len(tr) - 235, 1)))


def test_a_true_map_is_worth_the_corner_on_the_cpu(oracle):
    """path3 from sample int(0.50 M) at 8 m/s, 220 periods, base road mu = 1.0 with MU_SCALE 0.35 in the tight corner; plan row a_lat = 0.6 g, a_brake
    0.7, floor 1.0.  Every solve Optimal; largest |e_ct| with map = truth < 0.2 x without a plan; the neutral-map arm clips exactly as often as the
    arm without a plan; no period's nearest-sample margin below speed_plan_ref.MARGIN.
    Measured (printed): no plan 16.810 m, 11931 front sub-steps clipped, mean vx 11.28 m/s; plan with the neutral map 16.810 m, 11931, lowest v_plan
    7.849 m/s, mean vx 11.28; plan with map = truth 0.749 m, 1985, lowest v_plan 4.643 m/s, mean vx 8.43 (ratio 0.045); smallest margin of the three
    loops 2.4e-4 m^2."""
    res = {k: RP.cached_loop(oracle, k)[0] for k in ("no_plan", "neutral_map", "true_map")}
    for k, r in res.items():
        print("%-11s largest |e_ct| %.3f m, front sub-steps clipped %d, lowest v_plan %.3f m/s, mean vx %.2f m/s, smallest margin %.2e m^2"
              % (k, r["ect"].max(), r["stat"][0], r["v_plan"].min(), r["state"][:, 3].mean(), r["margin_min"]))
        assert (r["status"] == 0).all() and np.isfinite(r["state"]).all()
        assert not r["margin_low"] and r["margin_min"] >= SP.MARGIN
    e0, e1 = res["no_plan"]["ect"].max(), res["true_map"]["ect"].max()
    print("true map / no plan: %.3f" % (e1 / e0))
    assert e1 < 0.2 * e0
    assert res["neutral_map"]["stat"][0] == res["no_plan"]["stat"][0] and res["no_plan"]["stat"][0] > 0
    assert (res["no_plan"]["v_plan"] == SP.VT).all() and res["true_map"]["v_plan"].min() < res["neutral_map"]["v_plan"].min() < SP.VT
    # the plant drove on mu = 0.35 inside the patch and on mu = 1.0 outside it, in every arm
    for r in res.values():
        assert set(np.unique(r["road"][:, 0])) == {0.35, 1.0} and np.array_equal(r["road"][:, 0], r["road"][:, 1]) and (r["road"][:, 2:4] == 0.0).all()


def test_a_speed_zone_is_met_exactly_on_the_cpu(oracle):
    """a 4 m/s zone 60 ... 90 m ahead of the start, neutral road, a_lat = +inf: v_plan reaches exactly 4.0, every solve Optimal, no margin below MARGIN.
    Measured (printed): lowest v_plan 4.000 m/s, largest |e_ct| 0.129 m, mean vx 6.93 m/s, smallest margin 2.9e-4 m^2."""
    r = RP.cached_loop(oracle, "zone")[0]
    print("zone: lowest v_plan %.3f m/s, largest |e_ct| %.3f m, mean vx %.2f m/s, smallest margin %.2e m^2"
          % (r["v_plan"].min(), r["ect"].max(), r["state"][:, 3].mean(), r["margin_min"]))
    assert (r["status"] == 0).all() and not r["margin_low"]
    assert r["v_plan"].min() == 4.0 and (r["v_plan"] == 4.0).sum() >= 10 and r["v_plan"][0] == SP.VT and r["v_plan"][-1] == SP.VT
    assert (r["road"] == RR.NEUTRAL_ROW).all() and r["stat"][0] == 0


def test_a_stretch_of_bank_and_grade_acts_on_the_cpu(oracle):
    """A_LAT 1.5 and A_LONG -0.5 m/s^2 on the stretch 20 ... 60 m ahead of the start, 6 m/s, 150 periods, no plan: the plant's row carries the two
    words inside the stretch only; every solve Optimal; the loop is the neutral table's loop, bit for bit, up to the first period inside the stretch
    and differs from it in every later state.
    Measured (printed): largest |e_ct| 0.555 m with the stretch, 0.625 m on the neutral table (the corner later in the run, which the slowed vehicle
    reaches later); largest difference in position between the two loops 1.987 m; 60 periods inside from period 31; smallest margin 2.8e-4 m^2."""
    r, tr, i0 = RP.cached_loop(oracle, "stretch")
    a = RP.arms()["stretch"]
    flat_ = RP.cpu_loop(oracle, tr, i0, a["base"], np.tile(RP.NEUTRAL_ROW, (len(tr), 1)), steps=a["steps"], vt=a["vt"])
    inside = (r["road"][:, 3] == 1.5)
    k0 = int(np.argmax(inside))
    dpos = np.hypot(r["state"][:, 0] - flat_["state"][:, 0], r["state"][:, 1] - flat_["state"][:, 1])
    print("stretch: largest |e_ct| %.3f m (neutral table %.3f m), largest |dpos| between the two %.3f m, %d periods inside from period %d, smallest "
          "margin %.2e m^2" % (r["ect"].max(), flat_["ect"].max(), dpos.max(), inside.sum(), k0, r["margin_min"]))
    assert (r["status"] == 0).all() and not r["margin_low"]
    assert 30 <= inside.sum() <= 100 and np.array_equal(inside, r["road"][:, 2] == -0.5) and (r["road"][~inside, 2:4] == 0.0).all()
    assert not inside[0] and not inside[-1] and np.isinf(r["road"][:, 0:2]).all()
    assert np.array_equal(r["state"][:k0 + 1], flat_["state"][:k0 + 1]) and (r["state"][k0 + 1:, :6] != flat_["state"][k0 + 1:, :6]).all()
