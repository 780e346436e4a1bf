"""The road profile on the device: kmpc_road_profile_fleet and kmpc_speed_plan_fleet_profile against the numpy restatement tests/road_profile_ref.py
(which has no early exit), word by word, under bad vehicles and bad table words, and inside the closed loops (VehicleSimulator(road_profile=),
SpeedPlanner(profile=)).

Tolerances.  road_out, `closest`, w, d_bind and kappa_bind are exact: one _rn operation per word, an index reduction, a minimum.  v_plan and
sqrt(lim_i) pass through the device's fp64 sqrt: exact if it is correctly rounded, at most 1 ulp otherwise (the speed plan's bound); measured:
MEASURED_SQRT_ULP below.  The neutral-table tests are exact (torch.equal).  The loop against the CPU loop: 10 x the value measured on the MI355X,
capped at 1e-6 m / 1e-6 (the existing loop tests' rule); measured: MEASURED_LOOP below."""
import numpy as np
import pytest

import fleet_scenario as F
import road_profile_ref as RP
import road_ref as RR
import speed_plan_ref as SP

pytestmark = pytest.mark.gpu

# measured on the MI355X (2026-10-19): the largest difference, in units in the last place, of v_plan and of sqrt(lim_i) from numpy's sqrt over the 300-vehicle
# draw, and the same over the 128 early-exit vehicles: 0 in all four (the device's fp64 sqrt rounded as numpy's) -- see test_plan_with_a_map_matches_the_restatement_on_the_draw's docstring; bound: 1 ulp
MEASURED_SQRT_ULP = (0, 0)
# measured on the MI355X (2026-10-19): the three vehicles of the 150-period loop (true map, 4 m/s zone, bank / grade stretch) against the CPU loops, largest
# position difference [m], largest difference of the other states and the commands, largest difference of v_plan [m/s] -- see
# test_loop_matches_the_cpu_loops' docstring; bound = 10 x, capped at 1e-6; v_plan was identical in every period, so its bound is 10 x one ulp of 8 m/s
# (1.776e-15), as tests/test_speed_plan.py does
MEASURED_LOOP = (9.105e-11, 1.948e-10, 0.0)
TOL_LOOP = np.array([9.2e-10, 2.0e-9, 1.8e-14])

KEYS = ("v_plan", "w", "d_bind", "kappa_bind", "v_here", "closest")


def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64).cuda()


def ulps(a, b):
    """largest distance of a from b in units in the last place (finite doubles of one sign)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return int(np.abs(a.view(np.int64) - b.view(np.int64)).max()) if a.size else 0


def five_fleet(path_id):
    from mkz_mpc_path_follower_amd import FleetRefTrajectory
    return FleetRefTrajectory(F.five_paths(), path_id, traj_horizon=8, traj_dt=0.2)


def profile_on(grt, tab):
    """a RoadProfile of grt with the restatement's table (a list of [M_p,8]); tables with words check_road_profile refuses go in through copy_"""
    from mkz_mpc_path_follower_amd.vehicle_sim import RoadProfile
    prof = RoadProfile(grt)
    prof.table.copy_(dev(RP.flat(tab)))
    return prof


def run_plan(path_id, x, y, v_cap, rows, tab=None):
    """one plan() with info on the five paths, with the map `tab` (None: kmpc_speed_plan_fleet) -> dict of numpy arrays: KEYS and the waypoint
    kernel's closest"""
    import torch
    from mkz_mpc_path_follower_amd.ref_traj import SpeedPlanner
    B = len(path_id)
    grt = five_fleet(path_id)
    pl = SpeedPlanner(grt, window=SP.WINDOW, rows=dev(rows), profile=None if tab is None else profile_on(grt, tab))
    pose = dev(np.stack([x, y, np.zeros(B)], 1))
    v = pl.plan(pose, dev(v_cap), want_info=True)
    finite_pose = torch.where(torch.isfinite(pose), pose, torch.zeros_like(pose))
    _, _, wp_closest = grt.get_waypoints_batch(finite_pose, dev(np.full(B, 5.0)), want_closest=True)
    torch.cuda.synchronize()
    info = pl.info.cpu().numpy()
    return dict(v_plan=v.cpu().numpy(), w=info[:, 0], d_bind=info[:, 1], kappa_bind=info[:, 2], v_here=info[:, 3], closest=pl.closest.cpu().numpy(),
                wp_closest=wp_closest.cpu().numpy())


def run_compose(path_id, x, y, base, tab):
    """one RoadProfile.apply on the five paths -> (road_out [B,8], closest [B]) as numpy; the output buffer starts as NaN: every word is written"""
    import torch
    grt = five_fleet(path_id)
    prof = profile_on(grt, tab)
    out = dev(np.full((len(path_id), 8), np.nan))
    prof.apply(dev(np.stack([x, y], 1)), dev(base), out, want_closest=True)
    torch.cuda.synchronize()
    return out.cpu().numpy(), prof.closest.cpu().numpy()


def assert_matches(g, e, what):
    """device outputs g against the restatement's e: exact, the two sqrt words within 1 ulp -> their ulp distances"""
    assert np.isfinite(g["v_plan"]).all() and all(np.isfinite(g[k]).all() for k in ("w", "d_bind", "kappa_bind", "v_here")), what
    assert np.array_equal(g["closest"], e["closest"]), what
    for k in ("w", "d_bind", "kappa_bind"):
        assert np.array_equal(g[k], e[k]), (what, k, np.flatnonzero(g[k] != e[k])[:8])
    u = (ulps(g["v_plan"], e["v_plan"]), ulps(g["v_here"], e["v_here"]))
    assert max(u) <= 1, (what, u)
    return u


# ---------------------------------------------------------------- 1: compose against the restatement
def test_compose_matches_the_restatement_on_the_draw():
    """the 300-vehicle draw of tests/road_profile_ref.py (its branch counts are asserted in tests/test_road_profile_ref.py): road_out is exact, word
    for word, closest equals kmpc_waypoints_fleet's and the restatement's, and words 4 ... 7 of the base rows -- NaN, +inf and -inf among them in
    words 6, 7 -- pass through bit for bit"""
    import torch
    d = RP.draw()
    e_out, e_closest = RP.draw_compose()
    out, closest = run_compose(d["path_id"], d["x"], d["y"], d["road_base"], d["table"])
    grt = five_fleet(d["path_id"])
    _, _, wp_closest = grt.get_waypoints_batch(dev(np.stack([d["x"], d["y"], np.zeros(RP.DRAW_B)], 1)), dev(np.full(RP.DRAW_B, 5.0)), want_closest=True)
    torch.cuda.synchronize()
    assert np.array_equal(closest, e_closest) and np.array_equal(closest, wp_closest.cpu().numpy())
    assert np.array_equal(out[:, :4], e_out[:, :4]), np.flatnonzero((out[:, :4] != e_out[:, :4]).any(1))[:8]
    assert out[:, 4:8].tobytes() == d["road_base"][:, 4:8].tobytes()
    assert np.isnan(out[:, 6:8]).any() and np.isinf(out[:, 6:8]).any() and (out[:, :4] != d["road_base"][:, :4]).any(1).sum() >= 100


# ---------------------------------------------------------------- 2: the neutral table
def test_neutral_table_changes_nothing():
    """with the neutral table road_out torch.equal road_base (road_ref.random_rows: no -0.0 among them), and kmpc_speed_plan_fleet_profile torch.equal
    kmpc_speed_plan_fleet on speed_plan_ref.draw() in v_plan, all four info words and closest"""
    trajs = SP.five_trajectories()
    d = SP.draw()
    base = RR.random_rows(SP.DRAW_B, 5)
    out, closest = run_compose(d["path_id"], d["x"], d["y"], base, RP.table(trajs))
    assert out.tobytes() == base.tobytes() and (closest >= 0).all()
    a = run_plan(d["path_id"], d["x"], d["y"], d["v_cap"], d["rows"])
    b = run_plan(d["path_id"], d["x"], d["y"], d["v_cap"], d["rows"], RP.table(trajs))
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (b["v_plan"] < d["v_cap"]).sum() >= 40 and np.array_equal(closest, b["closest"])


# ---------------------------------------------------------------- 3: the plan with a map
def test_plan_with_a_map_matches_the_restatement_on_the_draw():
    """the 300-vehicle draw with its table: closest equals kmpc_waypoints_fleet's; w, d_bind and kappa_bind are exact; v_plan and sqrt(lim_i) within
    1 ulp.  Measured on the MI355X: v_plan and sqrt(lim_i) within 0 ulp of the restatement (MEASURED_SQRT_ULP); 172 of the 300 vehicles limited."""
    d, e = RP.draw(), RP.draw_plan()
    g = run_plan(d["path_id"], d["x"], d["y"], d["v_cap"], d["rows"], d["table"])
    assert np.array_equal(g["closest"], g["wp_closest"])
    u = assert_matches(g, e, "draw")
    print("draw: v_plan within %d ulp, sqrt(lim_i) within %d ulp of the restatement; %d vehicles limited" % (u[0], u[1], (g["v_plan"] < d["v_cap"]).sum()))


def early_exit_inputs():
    """test_speed_plan.test_early_exit_is_exact's 128 vehicles (64 with v_cap 40 and A_BRAKE 0.3, whose pass runs to the path's end, next to 64 with
    v_cap 2 and A_BRAKE 2, whose 1 m window ends inside the first chunk; starts at samples 0, 63, 64, 65, M - 65, M - 64 and M - 1 of path 0 in each
    group) on the draw's table with V_LIMIT = 0 at samples 30, 200 and M - 30 of path 0: inside the first chunk of the starts 0 and M - 65, M - 64,
    beyond it for 63, 64, 65"""
    trajs = SP.five_trajectories()
    rng = np.random.default_rng(5)
    M0 = len(trajs[0])
    fixed = [0, 63, 64, 65, M0 - 65, M0 - 64, M0 - 1]
    pid, idx = [], []
    for _ in range(2):
        pid += [0] * len(fixed)
        idx += fixed
        for k in range(64 - len(fixed)):
            p = SP.LONG[k % 3]
            pid.append(p)
            idx.append(int(rng.integers(0, len(trajs[p]))))
    pid, idx = np.array(pid, dtype=np.int32), np.array(idx)
    x = np.array([trajs[p][i, 4] for p, i in zip(pid, idx)])
    y = np.array([trajs[p][i, 5] for p, i in zip(pid, idx)])
    v_cap = np.repeat([40.0, 2.0], 64)
    rows = SP.rows(128, a_brake=np.repeat([0.3, 2.0], 64), end_stop=(np.arange(128) % 2 == 0).astype(np.float64))
    tab = [t.copy() for t in RP.draw()["table"]]
    tab[0][[30, 200, M0 - 30], 3] = 0.0
    return trajs, fixed, pid, x, y, v_cap, rows, tab


def test_early_exit_is_exact_with_a_map():
    """all exact against the restatement's full minimum; the V_LIMIT = 0 samples bind the fixed starts of the long-window group (jb 30 for start 0, 200
    for 63, 64, 65, M - 30 for M - 65 and M - 64).  Measured on the MI355X: 0 ulp in both sqrt words; 38 of the 64 long-window vehicles bound beyond
    one chunk."""
    trajs, fixed, pid, x, y, v_cap, rows, tab = early_exit_inputs()
    M0 = len(trajs[0])
    assert max(tr[-1, 6] for tr in trajs) < 40.0 ** 2 / (2 * 0.3)
    e = RP.plan(trajs, SP.five_kappas(), tab, pid, x, y, v_cap, rows)
    assert np.array_equal(e["closest"][:7], fixed) and e["jb"][:6].tolist() == [30, 200, 200, 200, M0 - 30, M0 - 30]
    assert (e["jb"][:64] - e["closest"][:64] > 64).sum() >= 10 and (e["d_bind"][64:] <= 1.0).all()
    g = run_plan(pid, x, y, v_cap, rows, tab)
    u = assert_matches(g, e, "early exit")
    print("early exit: v_plan within %d ulp, sqrt(lim_i) within %d ulp; %d bound beyond one chunk" % (u + ((e["jb"][:64] - e["closest"][:64] > 64).sum(),)))


# ---------------------------------------------------------------- 4: isolation and refusal
def test_a_paths_rows_reach_its_own_vehicles_only():
    """path 0's rows rewritten (MU_SCALE 0.3, A_LONG 0.7, A_LAT -1.1, V_LIMIT 1.5 everywhere): every vehicle on paths 1 ... 4 is bit-identical in both
    kernels, and vehicles of path 0 change in both"""
    d = RP.draw()
    tab2 = [t.copy() for t in d["table"]]
    tab2[0][:, :4] = (0.3, 0.7, -1.1, 1.5)
    other = d["path_id"] != 0
    a, b = run_plan(d["path_id"], d["x"], d["y"], d["v_cap"], d["rows"], d["table"]), run_plan(d["path_id"], d["x"], d["y"], d["v_cap"], d["rows"], tab2)
    for k in KEYS:
        assert a[k][other].tobytes() == b[k][other].tobytes(), k
    assert (a["v_plan"][~other] != b["v_plan"][~other]).sum() >= 30
    (ra, ca), (rb, cb) = (run_compose(d["path_id"], d["x"], d["y"], d["road_base"], t) for t in (d["table"], tab2))
    assert ra[other].tobytes() == rb[other].tobytes() and np.array_equal(ca, cb)
    assert (ra[~other, 2] != rb[~other, 2]).all()


def test_every_word_acts_on_its_own_consumer_only():
    """V_LIMIT does not reach road_out; A_LONG / A_LAT do not reach the plan; words 4 ... 7 reach nobody, NaN and inf included; MU_SCALE reaches both"""
    d = RP.draw()
    rng = np.random.default_rng(3)

    def changed(words, value):
        tab = [t.copy() for t in d["table"]]
        for t in tab:
            t[:, words] = value(t[:, words].shape)
        return tab
    args = (d["path_id"], d["x"], d["y"])
    plan0, (road0, _) = run_plan(*args, d["v_cap"], d["rows"], d["table"]), run_compose(*args, d["road_base"], d["table"])
    t_limit = changed([3], lambda s: rng.uniform(0.5, 3.0, s))
    t_force = changed([1, 2], lambda s: rng.uniform(-2.0, 2.0, s))
    t_mu = changed([0], lambda s: rng.uniform(0.1, 0.2, s))
    t_unread = changed([4, 5, 6, 7], lambda s: np.broadcast_to([np.nan, np.inf, -np.inf, 1e300], s))
    assert run_compose(*args, d["road_base"], t_limit)[0].tobytes() == road0.tobytes()
    assert run_compose(*args, d["road_base"], t_unread)[0].tobytes() == road0.tobytes()
    p_force, p_unread = run_plan(*args, d["v_cap"], d["rows"], t_force), run_plan(*args, d["v_cap"], d["rows"], t_unread)
    for k in KEYS:
        assert p_force[k].tobytes() == plan0[k].tobytes() and p_unread[k].tobytes() == plan0[k].tobytes(), k
    longp = np.isin(d["path_id"], SP.LONG)
    assert (run_plan(*args, d["v_cap"], d["rows"], t_limit)["v_plan"][longp] != plan0["v_plan"][longp]).sum() >= 100
    assert (run_compose(*args, d["road_base"], t_force)[0][:, 2:4] != road0[:, 2:4]).all()
    r_mu = run_compose(*args, d["road_base"], t_mu)[0]
    finite = np.isfinite(d["road_base"][:, 0])
    assert (r_mu[finite, 0] != road0[finite, 0]).all() and (run_plan(*args, d["v_cap"], d["rows"], t_mu)["v_plan"] != plan0["v_plan"]).sum() >= 30


BAD = ((11, "row", (0, np.nan)), (57, "row", (1, 0.0)), (90, "v_cap", -1.0), (123, "v_cap", np.nan), (188, "x", np.inf), (222, "path_id", -1),
       (299, "path_id", 5), (64, "row", (2, -0.5)), (65, "row", (3, np.nan)), (130, "y", np.nan), (131, "x", -np.inf), (132, "x", np.nan))
POSE_BAD = tuple(b for b, what, _ in BAD if what in ("x", "y", "path_id"))


def test_a_bad_vehicle_is_refused_alone():
    """twelve of the draw's 300 vehicles get one fault each (a NaN row word, A_BRAKE 0, v_cap -1, v_cap NaN, V_FLOOR < 0, END_STOP NaN; X = inf, -inf,
    NaN, Y NaN, path_id -1, path_id P).  The plan refuses all twelve (v_plan 0, info row 0, closest -1); the compose refuses the six with a bad pose or
    path_id and hands them their base row bit for bit, closest -1; every other vehicle is bit-identical to the run without them; every word the plan
    writes is finite"""
    d = RP.draw()
    pid, x, y, v_cap, rows = d["path_id"].copy(), d["x"].copy(), d["y"].copy(), d["v_cap"].copy(), d["rows"].copy()
    for b, what, v in BAD:
        if what == "row":
            rows[b, v[0]] = v[1]
        else:
            dict(v_cap=v_cap, x=x, y=y, path_id=pid)[what][b] = v
    good, g = run_plan(d["path_id"], d["x"], d["y"], d["v_cap"], d["rows"], d["table"]), run_plan(pid, x, y, v_cap, rows, d["table"])
    bad = np.array([b for b, _, _ in BAD])
    keep = np.ones(RP.DRAW_B, bool)
    keep[bad] = False
    for k in KEYS:
        assert np.isfinite(g[k]).all(), k
        assert g[k][keep].tobytes() == good[k][keep].tobytes(), k
        assert (g[k][bad] == (-1 if k == "closest" else 0.0)).all(), k
    e = RP.plan(SP.five_trajectories(), SP.five_kappas(), d["table"], pid, x, y, v_cap, rows)
    assert e["refused"][bad].all() and not e["refused"][keep].any()
    assert len(POSE_BAD) == 6
    (r0, c0), (r1, c1) = run_compose(d["path_id"], d["x"], d["y"], d["road_base"], d["table"]), run_compose(pid, x, y, d["road_base"], d["table"])
    keep = np.ones(RP.DRAW_B, bool)
    keep[list(POSE_BAD)] = False
    assert r1[keep].tobytes() == r0[keep].tobytes() and np.array_equal(c1[keep], c0[keep])
    assert r1[~keep].tobytes() == d["road_base"][~keep].tobytes() and (c1[~keep] == -1).all()
    e_out, e_closest = RP.compose(SP.five_trajectories(), d["table"], pid, x, y, d["road_base"])
    assert np.array_equal(c1, e_closest) and np.array_equal(r1[:, :4], e_out[:, :4])


@pytest.mark.parametrize("word", [0, 3])
def test_a_nan_table_word_refuses_only_the_vehicles_whose_pass_visits_it(word):
    """a NaN in MU_SCALE / V_LIMIT of sample jn of path 0 (jn = the restatement's closest of one of the draw's vehicles, so that someone stands on it):
    the vehicles of path 0 with jn - 64 < closest <= jn have it in their first chunk and are refused (v_plan 0, info row 0, closest -1); the vehicles
    behind it on path 0 (closest > jn) and everyone on another path are bit-identical to the run without it; a vehicle further before it is one or
    the other, according to where its exact early exit ends the pass (measured on the MI355X: none of those 27 was refused); every word written is
    finite.  In the compose the NaN reaches exactly the
    vehicles whose nearest sample is jn (MU_SCALE only)."""
    d, e = RP.draw(), RP.draw_plan()
    on0 = d["path_id"] == 0
    jn = int(np.sort(e["closest"][on0])[on0.sum() // 2])
    tab = [t.copy() for t in d["table"]]
    tab[0][jn, word] = np.nan
    good, g = run_plan(d["path_id"], d["x"], d["y"], d["v_cap"], d["rows"], d["table"]), run_plan(d["path_id"], d["x"], d["y"], d["v_cap"], d["rows"], tab)
    sure = on0 & (e["closest"] > jn - 64) & (e["closest"] <= jn)
    untouched = ~on0 | (e["closest"] > jn)
    maybe = ~sure & ~untouched
    assert sure.sum() >= 1 and untouched.sum() >= 240
    for k in KEYS:
        assert np.isfinite(g[k]).all(), k
        assert (g[k][sure] == (-1 if k == "closest" else 0.0)).all(), k
        assert g[k][untouched].tobytes() == good[k][untouched].tobytes(), k
    gone = g["closest"] == -1
    same = np.all([g[k] == good[k] for k in KEYS], 0)
    assert (gone | same)[maybe].all() and (gone[maybe] <= (g["v_plan"][maybe] == 0.0)).all()
    print("NaN in word %d of sample %d: %d refused for sure, %d of the %d further before it refused" % (word, jn, sure.sum(), gone[maybe].sum(), maybe.sum()))
    (r0, c0), (r1, c1) = run_compose(d["path_id"], d["x"], d["y"], d["road_base"], d["table"]), run_compose(d["path_id"], d["x"], d["y"], d["road_base"], tab)
    at = on0 & (c0 == jn)
    assert np.array_equal(c0, c1) and r1[~at].tobytes() == r0[~at].tobytes() and at.sum() >= 1
    assert np.isnan(r1[at, 0:2]).all() if word == 0 else r1[at].tobytes() == r0[at].tobytes()


# ---------------------------------------------------------------- 5: loops with a neutral profile
def _fleet_loop(vs, road_rows, with_profile, drive=False, planned=None):
    import torch
    import scenario as S
    from mkz_mpc_path_follower_amd import ClosedLoop, FleetRefTrajectory
    from mkz_mpc_path_follower_amd.ref_traj import SpeedPlanner, speed_plan_params
    from mkz_mpc_path_follower_amd.vehicle_sim import LowLevelController, RoadProfile, VehicleSimulator, drive_params
    B = len(vs)
    grt = FleetRefTrajectory([F.path_dict(p) for p in range(3)], [v["path"] for v in vs], time_mode=[0] * B, traj_horizon=F.N, traj_dt=0.2)
    kw = dict(road_profile=RoadProfile(grt)) if with_profile else {}
    if drive:
        kw.update(drive=drive_params(B), llc=LowLevelController(B, v0=np.array([v["v0"] for v in vs])))
    sim = VehicleSimulator(B, X0=np.array([v["X0"] for v in vs]), Y0=np.array([v["Y0"] for v in vs]), Psi0=np.array([v["Psi0"] for v in vs]),
                           road=dev(road_rows), **kw)
    sim.state[:, 3] = torch.as_tensor([v["v0"] for v in vs], dtype=torch.float64, device=sim.device)
    pl = None
    if planned is not None:
        pl = SpeedPlanner(grt, rows=speed_plan_params(B), profile=RoadProfile(grt) if planned else None)
    return ClosedLoop(grt, sim, N=F.N, target_vel=[v["target_vel"] for v in vs], weights=S.WEIGHTS, planner=pl), sim


@pytest.mark.parametrize("drive,steps", [(False, 40), (True, 20)])
def test_neutral_profile_leaves_the_loop_bit_for_bit(drive, steps):
    """vehicle kinds b ... e of fleet_scenario.vehicles() (12 vehicles on three paths) on road_ref.random_rows, 40 periods through
    kmpc_sim_advance_road and 20 through kmpc_sim_advance_drive: with road_profile= a neutral RoadProfile the state, cmd and status histories and
    road_stat are torch.equal to the loop on road= alone; sim.road is a tensor of its own next to sim.road_base, and equals it"""
    import torch
    vs = [v for v in F.vehicles() if v["kind"] in "bcde"]
    rows = RR.random_rows(12, 9)
    assert len(vs) == 12 and not ((rows[:, 2:4] == 0.0) & np.signbit(rows[:, 2:4])).any()
    (la, sa), (lb, sb) = _fleet_loop(vs, rows, False, drive), _fleet_loop(vs, rows, True, drive)
    a, b = la.run(steps, history=True), lb.run(steps, history=True)
    torch.cuda.synchronize()
    for k in ("state", "cmd", "status"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(sa.road_stat, sb.road_stat) and sa.road_stat[:, 2:4].max().item() > 0
    assert sa.road_base is None and sa.road_profile is None
    assert sb.road.data_ptr() != sb.road_base.data_ptr() and torch.equal(sb.road, sb.road_base) and torch.equal(sb.road_base.cpu(), torch.from_numpy(rows))


def test_neutral_map_leaves_the_planned_loop_bit_for_bit():
    """the same 12 vehicles, 40 periods, SpeedPlanner on the default rows with profile= a neutral RoadProfile against the planner without one: state,
    cmd, status and v_plan histories torch.equal, and the plan slows somebody down"""
    import torch
    vs = [v for v in F.vehicles() if v["kind"] in "bcde"]
    rows = RR.random_rows(12, 9)
    (la, _), (lb, _) = _fleet_loop(vs, rows, False, planned=False), _fleet_loop(vs, rows, False, planned=True)
    a, b = la.run(40, history=True), lb.run(40, history=True)
    torch.cuda.synchronize()
    for k in ("state", "cmd", "status", "v_plan"):
        assert torch.equal(a[k], b[k]), k
    assert la.planner.profile is None and lb.planner.profile is not None and (b["v_plan"] < lb.v_target).any().item()


# ---------------------------------------------------------------- 6: the loop against the CPU loops
LOOP_STEPS = 150
LOOP_ARMS = ("true_map", "zone", "stretch")


def _path3_fleet(B, copies=1):
    """B vehicles on `copies` copies of path3, vehicle b on copy b mod copies: a table per copy gives each vehicle a road of its own"""
    import scenario as S
    from mkz_mpc_path_follower_amd import FleetRefTrajectory
    arr, lat0, lon0 = S.path_arrays(SP.PATH)
    d = dict(arr)
    d.update(lat0=lat0, lon0=lon0)
    return FleetRefTrajectory([d] * copies, [b % copies for b in range(B)], traj_horizon=8, traj_dt=0.2)


def test_loop_matches_the_cpu_loops(oracle):
    """the true-map arm, the zone arm and the bank / grade stretch of tests/test_road_profile_ref.py as three vehicles of ONE ClosedLoop on three
    copies of path3 (a table per copy: the truth tables patch | neutral | stretch, the maps patch | zone | neutral; the stretch vehicle has no plan on
    the CPU and an unlimited row here: v_plan is its v_target, bit for bit), from sample int(0.50 M), 150 periods.  State, command and v_plan against
    road_profile_ref.cpu_loop by the 10 x rule (MEASURED_LOOP, TOL_LOOP, cap 1e-6); the clipped counts of both axles are exact; v_plan is identical in
    every period; every solve Optimal.
    Measured on the MI355X: true map 9.105e-11 m / 1.633e-10, zone 9.448e-13 m / 1.003e-11, stretch 9.122e-12 m / 1.948e-10 (positions / other states
    and commands); v_plan identical in all 150 periods of all three, lowest 4.643 / 4.000 / 6.000 m/s as in the CPU loops; clipped front sub-steps
    1985 / 0 / 0, rear 0, as in the CPU loops (none of which came near a limit without crossing it)."""
    import torch
    from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop
    from mkz_mpc_path_follower_amd.ref_traj import SpeedPlanner
    from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator
    arms = RP.arms()
    runs = [RP.cached_loop(oracle, k) for k in LOOP_ARMS]
    tr, i0 = runs[0][1], runs[0][2]
    a = [arms[k] for k in LOOP_ARMS]
    neutral = np.tile(RP.NEUTRAL_ROW, (len(tr), 1))
    grt = _path3_fleet(3, copies=3)
    truth = profile_on(grt, [x["truth"] for x in a])
    the_map = profile_on(grt, [x["map"] if x["map"] is not None else neutral for x in a])
    sim = VehicleSimulator(3, X0=np.full(3, tr[i0, 4]), Y0=np.full(3, tr[i0, 5]), Psi0=np.full(3, tr[i0, 3]), road=np.stack([x["base"] for x in a]),
                           road_profile=truth)
    vt = np.array([x["vt"] for x in a])
    sim.state[:, 3] = dev(vt)
    free = SP.rows(1, a_lat=np.inf, a_brake=SP.A_BRAKE, v_floor=SP.V_FLOOR)[0]
    pl = SpeedPlanner(grt, window=SP.WINDOW, rows=dev(np.stack([x["plan_row"] if x["plan_row"] is not None else free for x in a])), profile=the_map)
    loop = ClosedLoop(grt, sim, N=8, target_vel=vt.tolist(), planner=pl)
    out = loop.run(LOOP_STEPS, history=True)
    torch.cuda.synchronize()
    g = {k: out[k].cpu().numpy() for k in ("state", "cmd", "status", "latch", "v_plan")}
    stat = sim.road_stat.cpu().numpy()
    assert (g["status"] == 0).all() and not g["latch"].any() and np.isfinite(g["state"]).all() and (loop.score_summary()["n_nonopt"] == 0).all()
    worst = np.zeros(3)
    for b, (r, _, _) in enumerate(runs):
        assert (r["status"][:LOOP_STEPS] == 0).all() and not r["margin_low"]
        es, ec, ev = r["state"][:LOOP_STEPS + 1], r["cmd"][:LOOP_STEPS], r["v_plan"][:LOOP_STEPS]
        dp = np.hypot(g["state"][:, b, 0] - es[:, 0], g["state"][:, b, 1] - es[:, 1]).max()
        do = max(np.abs(g["state"][:, b, 2:] - es[:, 2:]).max(), np.abs(g["cmd"][:, b] - ec).max())
        dv = np.abs(g["v_plan"][:, b] - ev).max()
        print("vehicle %d (%s) against the CPU loop: max |dpos| %.3e m, other states and commands %.3e, v_plan %.3e m/s; lowest v_plan %.3f m/s "
              "(CPU %.3f); clipped sub-steps front / rear %d / %d (CPU %d / %d, near a limit: %s)"
              % (b, LOOP_ARMS[b], dp, do, dv, g["v_plan"][:, b].min(), ev.min(), stat[b, 0], stat[b, 1], r["stats"][LOOP_STEPS - 1, 0],
                 r["stats"][LOOP_STEPS - 1, 1], r["near"]))
        worst = np.maximum(worst, (dp, do, dv))
        assert np.array_equal(g["v_plan"][:, b], ev)
        assert np.array_equal(stat[b, 0:2], r["stats"][LOOP_STEPS - 1, 0:2])
    print("worst of the three: %s (bounds %s)" % (worst, TOL_LOOP))
    assert g["v_plan"][:, 0].min() < 5.0 and g["v_plan"][:, 1].min() == 4.0 and (g["v_plan"][:, 2] == RP.STRETCH_VT).all() and stat[0, 0] > 0
    assert (worst <= TOL_LOOP).all() and TOL_LOOP.max() <= 1e-6


# ---------------------------------------------------------------- 7: the map against no map on the device
def test_a_true_map_is_worth_the_corner_on_the_device():
    """48 vehicles on path3 at 8 m/s, on the path at samples int(0.50 M) + k (all before the tight corner), base road mu = 1.0 with MU_SCALE 0.35 in
    the corner (road_profile_ref.corner_patch), plan rows a_lat = 0.6 g, 220 periods: the fleet's largest |e_ct| with profile= the truth is below
    0.2 x that with the neutral map (the ratio of tests/test_road_profile_ref.py; the CPU loop gives 0.045); every solve Optimal.
    Measured on the MI355X: largest |e_ct| per vehicle 16.524 ... 16.927 m with the neutral map, 0.676 ... 0.901 m with the true map (ratio of the
    largest 0.053); lowest v_plan 7.849 / 4.643 m/s; front sub-steps clipped 11931 ... 12226 / 1897 ... 2131."""
    import torch
    from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop
    from mkz_mpc_path_follower_amd.ref_traj import SpeedPlanner, speed_plan_params
    from mkz_mpc_path_follower_amd.vehicle_sim import RoadProfile, VehicleSimulator, road_params
    _, _, _, tr, i0 = SP.loop_start()
    idx = i0 + np.arange(48)
    truth, patch = RP.corner_patch(tr)
    assert tr[idx[-1], 6] < tr[patch[0], 6] - 20.0
    res = []
    for knows in (False, True):
        grt = _path3_fleet(48)
        sim = VehicleSimulator(48, X0=tr[idx, 4], Y0=tr[idx, 5], Psi0=tr[idx, 3], road=road_params(48, mu=1.0), road_profile=RoadProfile(grt, truth))
        sim.state[:, 3] = SP.VT
        pl = SpeedPlanner(grt, window=SP.WINDOW, rows=speed_plan_params(48, a_lat=0.6 * RR.G, a_brake=SP.A_BRAKE, v_floor=SP.V_FLOOR),
                          profile=RoadProfile(grt, truth if knows else None))
        loop = ClosedLoop(grt, sim, N=8, target_vel=SP.VT, planner=pl)
        out = loop.run(RP.PERIODS, history=True)
        torch.cuda.synchronize()
        assert torch.isfinite(out["state"]).all().item() and (out["status"] == 0).all().item()
        res.append((loop.score_summary()["max_ect"], out["v_plan"].min().item(), sim.road_summary()["sat_f"]))
    (e0, v0, c0), (e1, v1, c1) = res
    print("largest |e_ct| per vehicle: neutral map %.3f ... %.3f m, true map %.3f ... %.3f m (ratio of the largest %.3f); lowest v_plan %.3f / %.3f m/s; "
          "front sub-steps clipped %d ... %d / %d ... %d" % (e0.min(), e0.max(), e1.min(), e1.max(), e1.max() / e0.max(), v0, v1, c0.min(), c0.max(),
                                                            c1.min(), c1.max()))
    assert e1.max() < 0.2 * e0.max()
