"""TEST INFRASTRUCTURE: numpy restatement of the speed plan (kmpc_pathset_curvature, kmpc_speed_plan_fleet), written from the text of include/kmpc.h,
not from the kernels; the committed 300-vehicle draw that tests/test_speed_plan_ref.py and tests/test_speed_plan.py share; and the one-vehicle CPU
loop with the plan in front of the waypoints and of the solver's v_target (road_ref.cpu_loop's shape, with a start index, a target speed and plan rows).

`plan` is the FULL minimum over all j >= i with np.argmin: it has no early exit, so it checks the kernel's.
"""
import numpy as np

import fleet_scenario as F
import plant_ref as R
import road_ref as RR
import track_score_ref as TS

FIELDS = ("a_lat", "a_brake", "v_floor", "end_stop")
DEFAULT_ROW = np.array([2.0, 0.7, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0])
WINDOW = 4.0


def rows(B, **kw):
    """[B,8] plan rows: the default, with any of FIELDS a scalar or one value per vehicle"""
    r = np.tile(DEFAULT_ROW, (B, 1))
    for k, v in kw.items():
        r[:, FIELDS.index(k)] = v
    return r


def curvature(traj, window):
    """traj [M,7] (t, lat, lon, psi, X, Y, cdist) -> kappa [M]: the recorded heading's difference over the arclength window, inside this path only"""
    s, psi = traj[:, 6], traj[:, 3]
    h = 0.5 * window
    ia = np.searchsorted(s, s - h, side="left")
    ib = np.searchsorted(s, s + h, side="right") - 1
    den = s[ib] - s[ia]
    num = TS.fix_heading(psi[ib] - psi[ia])
    with np.errstate(all="ignore"):
        return np.where(den > 0.0, num / np.where(den > 0.0, den, 1.0), 0.0), den


def nearest(traj, x, y):
    """the waypoint helper's argmin (first occurrence)"""
    return int(np.argmin((traj[:, 4] - x) ** 2 + (traj[:, 5] - y) ** 2))


def refused(P, path_id, x, y, v_cap, row):
    """the refusal conditions that need no sample (include/kmpc.h); a non-finite w is plan()'s own"""
    a_lat, a_brake, v_floor, end_stop = row[0:4]
    with np.errstate(invalid="ignore"):
        ok = (0 <= path_id < P and np.isfinite(x) and np.isfinite(y) and np.isfinite(v_cap) and v_cap >= 0.0 and a_lat > 0.0 and a_brake > 0.0
              and np.isfinite(a_brake) and v_floor >= 0.0 and np.isfinite(v_floor) and not np.isnan(end_stop))
    return not ok


REFUSED = dict(v_plan=0.0, w=0.0, d_bind=0.0, kappa_bind=0.0, v_here=0.0, closest=-1, jb=-1, refused=True)


def plan_one(traj, kappa, x, y, v_cap, row, i=None):
    """ONE vehicle on its own path -> dict v_plan, w, d_bind, kappa_bind, v_here, closest, jb, refused"""
    a_lat, a_brake, v_floor, end_stop = (np.float64(v) for v in row[0:4])
    s = traj[:, 6]
    M = len(s)
    i = nearest(traj, x, y) if i is None else i
    v_cap = np.float64(v_cap)
    with np.errstate(all="ignore"):
        vcap2 = v_cap * v_cap
        lim = np.minimum(vcap2, a_lat / np.maximum(np.fabs(kappa[i:]), 1e-9))
        if end_stop != 0.0:
            lim[M - 1 - i] = 0.0
        c = lim + (2.0 * a_brake) * (s[i:] - s[i])
        k = int(np.argmin(c))
        w = c[k]
        if not np.isfinite(w):
            return dict(REFUSED)
        v_plan = v_cap if w == vcap2 else min(v_cap, max(v_floor, np.sqrt(w)))
    return dict(v_plan=float(v_plan), w=float(w), d_bind=float(s[i + k] - s[i]), kappa_bind=float(kappa[i + k]), v_here=float(np.sqrt(lim[0])),
                closest=i, jb=i + k, refused=False)


def plan(trajs, kappas, path_id, x, y, v_cap, rows_):
    """B vehicles -> dict of arrays (plan_one's keys)"""
    out = []
    for b in range(len(path_id)):
        if refused(len(trajs), int(path_id[b]), x[b], y[b], v_cap[b], rows_[b]):
            out.append(dict(REFUSED))
        else:
            p = int(path_id[b])
            out.append(plan_one(trajs[p], kappas[p], x[b], y[b], v_cap[b], rows_[b]))
    return {k: np.array([o[k] for o in out]) for k in REFUSED}


# ---------------------------------------------------------------- the five paths and the committed draw
_cache = {}


def five_trajectories():
    """[M,7] arrays of fleet_scenario.five_paths(), from the oracle's restatement of the constructor"""
    if "five" not in _cache:
        from oracle import waypoints as W
        _cache["five"] = [W.build_trajectory(d["t"], d["lat"], d["lon"], d["psi"], d["lat0"], d["lon0"]) for d in F.five_paths()]
    return _cache["five"]


def five_kappas(window=WINDOW):
    if ("kappa", window) not in _cache:
        _cache[("kappa", window)] = [curvature(tr, window)[0] for tr in five_trajectories()]
    return _cache[("kappa", window)]


DRAW_SEED, DRAW_B = 77, 300
LONG = (0, 2, 4)     # the long paths of five_paths()


def draw(B=DRAW_B, seed=DRAW_SEED):
    """the committed draw: path ids interleaved 0 ... 4, a random sample of the vehicle's path +- 0.5 m, v_cap U(2, 12), A_LAT U(0.5, 4), A_BRAKE U(0.3, 2),
    V_FLOOR U(0, 2), END_STOP on for half.  Half of the long-path vehicles are placed within 60 m before a sample with |kappa| > 0.05 (so that
    curvature ahead binds), and every tenth vehicle of a long path within the last 40 m (so that END_STOP and the last chunk bind).
    -> dict path_id [B], x, y, v_cap [B], rows [B,8]"""
    if ("draw", B, seed) in _cache:
        return _cache[("draw", B, seed)]
    rng = np.random.default_rng(seed)
    trajs, kappas = five_trajectories(), five_kappas()
    pid = np.arange(B, dtype=np.int32) % 5
    x, y = np.zeros(B), np.zeros(B)
    n_long = 0
    for b in range(B):
        tr, kap = trajs[pid[b]], kappas[pid[b]]
        M = len(tr)
        i = int(rng.integers(0, M))
        if pid[b] in LONG:
            n_long += 1
            s = tr[:, 6]
            if n_long % 10 == 0:
                i = int(rng.choice(np.flatnonzero(s >= s[-1] - 40.0)))
            elif n_long % 2 == 0:
                tight = np.flatnonzero(np.fabs(kap) > 0.05)
                j = int(rng.choice(tight))
                i = int(rng.choice(np.flatnonzero((s <= s[j]) & (s >= s[j] - 60.0))))
        x[b], y[b] = tr[i, 4] + rng.uniform(-0.5, 0.5), tr[i, 5] + rng.uniform(-0.5, 0.5)
    r = np.tile(DEFAULT_ROW, (B, 1))
    v_cap = rng.uniform(2.0, 12.0, B)
    r[:, 0], r[:, 1], r[:, 2] = rng.uniform(0.5, 4.0, B), rng.uniform(0.3, 2.0, B), rng.uniform(0.0, 2.0, B)
    r[:, 3] = (rng.random(B) < 0.5).astype(np.float64)
    _cache[("draw", B, seed)] = dict(path_id=pid, x=x, y=y, v_cap=v_cap, rows=r)
    return _cache[("draw", B, seed)]


def draw_plan():
    """the restatement's plan of the committed draw, computed once per process"""
    if "draw_plan" not in _cache:
        d = draw()
        _cache["draw_plan"] = plan(five_trajectories(), five_kappas(), d["path_id"], d["x"], d["y"], d["v_cap"], d["rows"])
    return _cache["draw_plan"]


# ---------------------------------------------------------------- the closed loop of the issue's table
VT, N_UPD, PATH, AT, PERIODS = 8.0, 10, "path3_decimated.npz", 0.50, 220
LOOP_ROADS = (dict(), dict(mu=0.5), dict(mu=0.35))     # neutral, mu = 0.5, mu = 0.35
A_BRAKE, V_FLOOR = 0.7, 1.0
MARGIN = 1e-6     # a nearest-sample margin (second-smallest minus smallest squared distance) below this may pick another sample on the device


def plan_row(road_kw):
    """a_lat = 0.6 mu g (2.0 on the neutral road), a_brake 0.7, v_floor 1.0, no end stop"""
    mu = road_kw.get("mu")
    return rows(1, a_lat=2.0 if mu is None else 0.6 * mu * RR.G, a_brake=A_BRAKE, v_floor=V_FLOOR)[0]


def loop_start(start=None):
    """the path's sample int(AT * M) (or `start`) and its heading -> X0, Y0, Psi0, trajectory, start index"""
    from oracle import waypoints as W
    import scenario as S
    arr, lat0, lon0 = S.path_arrays(PATH)
    tr = W.build_trajectory(arr["t"], arr["lat"], arr["lon"], arr["psi"], lat0, lon0)
    i = int(AT * len(tr)) if start is None else int(start)
    return tr[i, 4], tr[i, 5], tr[i, 3], tr, i


def cpu_loop(O, traj, start, road_row, plan_row_=None, steps=PERIODS, vt=VT, window=WINDOW, weights=None):
    """road_ref.cpu_loop with a start INDEX (the vehicle starts on the path at sample `start`, at its heading, already at `vt`), a target speed, and,
    with plan_row_ given, the plan in front of W.get_waypoints and of O.problem's v_target (v_cap = vt, planned on the truth).
    -> road_ref.cpu_loop's dict, plus v_plan [steps] and margin_low (bool: some period's nearest-sample margin fell below MARGIN)"""
    from oracle import waypoints as W, vehicle_sim as Vs
    import scenario as S
    p = O.params(8, weights if weights is not None else S.WEIGHTS)
    s = Vs.initial_state(1, traj[start, 4], traj[start, 5], traj[start, 3])
    s[0, 3] = vt
    plant, road = R.DEFAULT_ROW[None, :], np.asarray(road_row, dtype=np.float64)[None, :]
    kappa = curvature(traj, window)[0] if plan_row_ is not None else None
    u_prev, U_prev, have_warm = np.zeros(2), None, False
    cmds, states, status, v_plan = np.zeros((steps, 1, 2)), np.zeros((steps + 1, 1, 8)), [], np.full(steps, vt)
    states[0] = s
    stat, near = np.zeros((1, 4)), np.zeros(1, dtype=bool)
    margin_low = False
    for k in range(steps):
        x, y, psi, v = s[0, 0:4]
        d2 = np.sort((traj[:, 4] - x) ** 2 + (traj[:, 5] - y) ** 2)
        margin_low |= bool(d2[1] - d2[0] < MARGIN)
        if plan_row_ is not None:
            v_plan[k] = plan_one(traj, kappa, x, y, vt, plan_row_)["v_plan"]
        xr, yr, pr, _stop, _ci = W.get_waypoints(traj, x, y, psi, v_plan[k], traj_horizon=8)
        q = O.problem(p, [x, y, psi, v], np.stack([xr, yr, pr], 1), v_plan[k], u_prev)
        r = O.solve_condensed(p, q, o=O.opts(warm=1) if have_warm else O.opts(), U0=U_prev)
        cmd = r["U"][0].copy()
        u_prev, U_prev, have_warm = cmd.copy(), r["U"].copy(), True
        cmds[k, 0] = cmd
        status.append(r["status"])
        s, stat = RR.advance_road(s, cmds, k, plant, road, [0], 2, N_UPD, stat=stat, near=near)
        states[k + 1] = s
    ect, _ = S.cross_track(traj[:, 4:6], states[:, 0, 0], states[:, 0, 1])
    return dict(state=states[:, 0], cmd=cmds[:, 0], status=np.array(status), stat=stat[0], near=bool(near[0]), ect=ect, v_plan=v_plan,
                margin_low=margin_low)


START_SHIFT = (0, 0, 0)     # samples added to int(AT * M) per road, so that no period's nearest-sample margin falls below MARGIN (none needed)


def cached_loop(O, ri, planned, steps=PERIODS):
    """road ri of LOOP_ROADS, plain or planned, computed once per process -> cpu_loop's dict of AT LEAST `steps` periods (the loop is deterministic: a
    shorter run is a longer one's beginning, so the caller slices), trajectory, start index"""
    _, _, _, tr, i0 = loop_start()
    key = ("loop", ri, planned)
    if key not in _cache or len(_cache[key]["cmd"]) < steps:
        kw = LOOP_ROADS[ri]
        _cache[key] = cpu_loop(O, tr, i0 + START_SHIFT[ri], RR.rows(1, **kw)[0], plan_row(kw) if planned else None, steps=steps)
    return _cache[key], tr, i0 + START_SHIFT[ri]
