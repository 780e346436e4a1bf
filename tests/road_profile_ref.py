"""TEST INFRASTRUCTURE: numpy restatement of the road profile (kmpc_road_profile_fleet, kmpc_speed_plan_fleet_profile), written from the text of
include/kmpc.h, not from the kernels; the committed 300-vehicle draw with its table that tests/test_road_profile_ref.py and tests/test_road_profile.py
share; and the one-vehicle CPU loop (speed_plan_ref.cpu_loop's shape) in which the plant's road row is composed from the TRUTH table at the truth's
nearest sample before every advance_road, and the plan reads its own table, the MAP.

A table here is a list of per-path arrays [M_p, 8]; `flat` concatenates them into the device's [sum M, 8].
`plan` is the FULL minimum over all j >= i with np.argmin: it has no early exit, so it checks the kernel's.
"""
import numpy as np

import plant_ref as R
import road_ref as RR
import speed_plan_ref as SP

FIELDS = ("mu_scale", "a_long", "a_lat", "v_limit")
NEUTRAL_ROW = np.array([1.0, 0.0, 0.0, np.inf, 0.0, 0.0, 0.0, 0.0])


def table(trajs):
    """the neutral table of these paths: a list of [M_p,8]"""
    return [np.tile(NEUTRAL_ROW, (len(tr), 1)) for tr in trajs]


def flat(tab):
    return np.ascontiguousarray(np.concatenate(tab, 0))


def patch(prof, traj, s0, s1, **words):
    """writes the words given into the rows of ONE path's table whose sample has cdist in [s0, s1] -> the indices written"""
    s = traj[:, 6]
    idx = np.flatnonzero((s >= s0) & (s <= s1))
    for k, v in words.items():
        prof[idx, FIELDS.index(k)] = v
    return idx


# ---------------------------------------------------------------- compose: kmpc_road_profile_fleet
def compose_row(base, r):
    """road_base row [8] and a profile row [8] -> road_out row [8]; words 4 ... 7 are base's own"""
    out = np.array(base, dtype=np.float64, copy=True)
    with np.errstate(all="ignore"):
        out[0] = base[0] * r[0]
        out[1] = base[1] * r[0]
        out[2] = base[2] + r[1]
        out[3] = base[3] + r[2]
    return out


def compose(trajs, tab, path_id, x, y, base):
    """B vehicles -> (road_out [B,8], closest [B]); a refused vehicle (path_id outside the set, non-finite X or Y) keeps its base row, closest -1"""
    out = np.array(base, dtype=np.float64, copy=True)
    closest = np.full(len(path_id), -1, dtype=np.int32)
    for b in range(len(path_id)):
        p = int(path_id[b])
        if not (0 <= p < len(trajs) and np.isfinite(x[b]) and np.isfinite(y[b])):
            continue
        closest[b] = SP.nearest(trajs[p], x[b], y[b])
        out[b] = compose_row(base[b], tab[p][closest[b]])
    return out, closest


# ---------------------------------------------------------------- the plan with a map: kmpc_speed_plan_fleet_profile
REFUSED = dict(SP.REFUSED, kind=-1)
CAP, CORNER, LIMIT, END = 0, 1, 2, 3     # which term is the binding sample's limit


def plan_one(traj, kappa, prof, x, y, v_cap, row, i=None):
    """speed_plan_ref.plan_one with the map `prof` [M,8] of the vehicle's own path -> its keys, plus kind (CAP, CORNER, LIMIT or END at sample jb)"""
    a_lat, a_brake, v_floor, end_stop = (np.float64(v) for v in row[0:4])
    s = traj[:, 6]
    M = len(s)
    i = SP.nearest(traj, x, y) if i is None else i
    v_cap = np.float64(v_cap)
    with np.errstate(all="ignore"):
        vcap2 = v_cap * v_cap
        a = a_lat * prof[i:, 0]
        q = a / np.maximum(np.fabs(kappa[i:]), 1e-9)
        vl2 = prof[i:, 3] * prof[i:, 3]
        lim = np.minimum(np.minimum(vcap2, q), vl2)
        if end_stop != 0.0:
            lim[M - 1 - i] = 0.0
        c = lim + (2.0 * a_brake) * (s[i:] - s[i])
        k = int(np.argmin(c))
        w = c[k]
        if not np.isfinite(w):
            return dict(REFUSED)
        v_plan = v_cap if w == vcap2 else min(v_cap, max(v_floor, np.sqrt(w)))
        kind = END if (end_stop != 0.0 and i + k == M - 1) else (LIMIT if vl2[k] < min(vcap2, q[k]) else (CORNER if q[k] < vcap2 else CAP))
    return dict(v_plan=float(v_plan), w=float(w), d_bind=float(s[i + k] - s[i]), kappa_bind=float(kappa[i + k]), v_here=float(np.sqrt(lim[0])),
                closest=i, jb=i + k, refused=False, kind=kind)


def plan(trajs, kappas, tab, path_id, x, y, v_cap, rows_):
    """B vehicles -> dict of arrays (plan_one's keys)"""
    out = []
    for b in range(len(path_id)):
        if SP.refused(len(trajs), int(path_id[b]), x[b], y[b], v_cap[b], rows_[b]):
            out.append(dict(REFUSED))
        else:
            p = int(path_id[b])
            out.append(plan_one(trajs[p], kappas[p], tab[p], x[b], y[b], v_cap[b], rows_[b]))
    return {k: np.array([o[k] for o in out]) for k in REFUSED}


# ---------------------------------------------------------------- the committed draw
_cache = {}
DRAW_SEED, DRAW_B = 91, 300
ZERO_LEN, ZONE_LEN, PATCH_LEN, STRETCH_LEN = 3.0, 25.0, 30.0, 50.0


def draw_table(seed=DRAW_SEED):
    """the committed table on fleet_scenario.five_paths().  On each long path, at random places: 6 MU_SCALE patches U(0.25, 0.9) of 30 m, four of them
    centred on a sample with |kappa| > 0.04; 5 V_LIMIT zones U(1, 6) m/s of 25 m; 2 zones of 3 m with V_LIMIT exactly 0; 4 stretches of 50 m with A_LONG
    U(-1, 1) and A_LAT U(-2, 2); words 4 ... 7 of every row of path 0 are U(-9, 9) (read by nobody).  The short paths (M = 2, M = 65) stay neutral but
    for one V_LIMIT 3.0 sample in the middle of the M = 65 path.
    -> (table: list of [M_p,8], marks: per long path a dict of the arclengths at which the mu patches, the zones and the zero zones begin)"""
    if ("table", seed) in _cache:
        return _cache[("table", seed)]
    rng = np.random.default_rng(seed)
    trajs, kappas = SP.five_trajectories(), SP.five_kappas()
    tab = table(trajs)
    marks = {}
    for p in SP.LONG:
        tr, kap = trajs[p], kappas[p]
        s = tr[:, 6]
        L = s[-1]
        tight = np.flatnonzero(np.fabs(kap) > 0.04)
        m = dict(mu=[], zone=[], zero=[])
        for k in range(6):
            c = s[int(rng.choice(tight))] if (k % 3 != 2 and len(tight)) else rng.uniform(0.0, L)
            patch(tab[p], tr, c - 0.5 * PATCH_LEN, c + 0.5 * PATCH_LEN, mu_scale=rng.uniform(0.25, 0.9))
            m["mu"].append(c - 0.5 * PATCH_LEN)
        for k in range(5):
            a = rng.uniform(0.1 * L, 0.95 * L)
            patch(tab[p], tr, a, a + ZONE_LEN, v_limit=rng.uniform(1.0, 6.0))
            m["zone"].append(a)
        for k in range(2):
            a = rng.uniform(0.2 * L, 0.9 * L)
            patch(tab[p], tr, a, a + ZERO_LEN, v_limit=0.0)
            m["zero"].append(a)
        for k in range(4):
            a = rng.uniform(0.0, L)
            patch(tab[p], tr, a, a + STRETCH_LEN, a_long=rng.uniform(-1.0, 1.0), a_lat=rng.uniform(-2.0, 2.0))
        marks[p] = m
    tab[0][:, 4:8] = rng.uniform(-9.0, 9.0, (len(tab[0]), 4))
    tab[3][32, 3] = 3.0
    _cache[("table", seed)] = (tab, marks)
    return _cache[("table", seed)]


def draw(B=DRAW_B, seed=DRAW_SEED):
    """the committed draw: path ids interleaved 0 ... 4; v_cap U(2, 12), A_LAT U(0.5, 4), A_BRAKE U(0.3, 2), V_FLOOR U(0, 2), END_STOP on for half
    (speed_plan_ref.draw's ranges); road_base rows road_ref.random_rows' with NaN / inf payloads in words 6, 7.  Long-path vehicles by turns: within
    80 m before a V_LIMIT zone, within 80 m before a V_LIMIT 0 zone, within 60 m before a MU_SCALE patch, inside a MU_SCALE patch, from 30 m before a
    MU_SCALE patch to its middle, at a random sample; all +- 0.5 m off their sample.
    -> dict path_id [B], x, y, v_cap [B], rows [B,8], road_base [B,8], table (list of [M_p,8])"""
    if ("draw", B, seed) in _cache:
        return _cache[("draw", B, seed)]
    tab, marks = draw_table(seed)
    rng = np.random.default_rng(seed + 1)
    trajs = SP.five_trajectories()
    pid = np.arange(B, dtype=np.int32) % 5
    x, y = np.zeros(B), np.zeros(B)
    n_long = 0
    for b in range(B):
        tr = trajs[pid[b]]
        s = tr[:, 6]
        i = int(rng.integers(0, len(tr)))
        if pid[b] in SP.LONG:
            m = marks[int(pid[b])]
            turn = n_long % 6
            n_long += 1
            if turn < 5:
                a = float(rng.choice(m[("zone", "zero", "mu", "mu", "mu")[turn]]))
                lo, hi = ((a - 80.0, a), (a - 80.0, a), (a - 60.0, a), (a, a + PATCH_LEN), (a - 30.0, a + 0.5 * PATCH_LEN))[turn]
                cand = np.flatnonzero((s >= lo) & (s <= hi))
                if len(cand):
                    i = int(rng.choice(cand))
        x[b], y[b] = tr[i, 4] + rng.uniform(-0.5, 0.5), tr[i, 5] + rng.uniform(-0.5, 0.5)
    r = np.tile(SP.DEFAULT_ROW, (B, 1))
    v_cap = rng.uniform(2.0, 12.0, B)
    r[:, 0], r[:, 1], r[:, 2] = rng.uniform(0.5, 4.0, B), rng.uniform(0.3, 2.0, B), rng.uniform(0.0, 2.0, B)
    r[:, 3] = (rng.random(B) < 0.5).astype(np.float64)
    base = RR.random_rows(B, seed + 2)
    base[0::3, 6], base[1::3, 6], base[2::3, 7], base[0::4, 7] = np.nan, np.inf, -np.inf, np.nan
    base[5::7, 2] = -0.0
    _cache[("draw", B, seed)] = dict(path_id=pid, x=x, y=y, v_cap=v_cap, rows=r, road_base=base, table=tab)
    return _cache[("draw", B, seed)]


def draw_plan():
    """the restatement's plan of the committed draw on its table, computed once per process"""
    if "draw_plan" not in _cache:
        d = draw()
        _cache["draw_plan"] = plan(SP.five_trajectories(), SP.five_kappas(), d["table"], d["path_id"], d["x"], d["y"], d["v_cap"], d["rows"])
    return _cache["draw_plan"]


def draw_compose():
    if "draw_compose" not in _cache:
        d = draw()
        _cache["draw_compose"] = compose(SP.five_trajectories(), d["table"], d["path_id"], d["x"], d["y"], d["road_base"])
    return _cache["draw_compose"]


# ---------------------------------------------------------------- the closed loops of the issue's table
PERIODS = SP.PERIODS
MU_PATCH, KAPPA_PATCH, PATCH_REACH = 0.35, 0.03, 10.0
ZONE = (60.0, 90.0, 4.0)                 # from, to [m ahead of the start], V_LIMIT [m/s]
STRETCH = (20.0, 60.0, 1.5, -0.5)        # from, to [m ahead of the start], A_LAT, A_LONG [m/s^2]
STRETCH_VT, STRETCH_PERIODS = 6.0, 150


def corner_patch(traj, mu_scale=MU_PATCH, window=SP.WINDOW):
    """a neutral table of ONE path with MU_SCALE = mu_scale on the samples within PATCH_REACH m of arclength of a sample with |kappa| >= KAPPA_PATCH
    -> ([M,8], the indices written)"""
    kap = SP.curvature(traj, window)[0]
    s = traj[:, 6]
    st = s[np.fabs(kap) >= KAPPA_PATCH]
    k = np.searchsorted(st, s)
    near = np.minimum(np.abs(s - st[np.clip(k - 1, 0, len(st) - 1)]), np.abs(s - st[np.clip(k, 0, len(st) - 1)])) <= PATCH_REACH
    prof = np.tile(NEUTRAL_ROW, (len(traj), 1))
    prof[near, 0] = mu_scale
    return prof, np.flatnonzero(near)


def arms():
    """the loops of the issue's table on path3 from sample int(0.50 M): name -> dict(base road row, truth table, plan row or None, map table or None,
    vt, steps)"""
    if "arms" in _cache:
        return _cache["arms"]
    _, _, _, tr, i0 = SP.loop_start()
    s0 = tr[i0, 6]
    neutral = np.tile(NEUTRAL_ROW, (len(tr), 1))
    truth, _ = corner_patch(tr)
    zone = neutral.copy()
    patch(zone, tr, s0 + ZONE[0], s0 + ZONE[1], v_limit=ZONE[2])
    stretch = neutral.copy()
    patch(stretch, tr, s0 + STRETCH[0], s0 + STRETCH[1], a_lat=STRETCH[2], a_long=STRETCH[3])
    grip = SP.rows(1, a_lat=0.6 * RR.G, a_brake=SP.A_BRAKE, v_floor=SP.V_FLOOR)[0]
    free = SP.rows(1, a_lat=np.inf, a_brake=SP.A_BRAKE, v_floor=SP.V_FLOOR)[0]
    wet, dry = RR.rows(1, mu=1.0)[0], RR.rows(1)[0]
    _cache["arms"] = dict(
        no_plan=dict(base=wet, truth=truth, plan_row=None, map=None, vt=SP.VT, steps=PERIODS),
        neutral_map=dict(base=wet, truth=truth, plan_row=grip, map=neutral, vt=SP.VT, steps=PERIODS),
        true_map=dict(base=wet, truth=truth, plan_row=grip, map=truth, vt=SP.VT, steps=PERIODS),
        zone=dict(base=dry, truth=neutral, plan_row=free, map=zone, vt=SP.VT, steps=PERIODS),
        stretch=dict(base=dry, truth=stretch, plan_row=None, map=None, vt=STRETCH_VT, steps=STRETCH_PERIODS))
    return _cache["arms"]


def cpu_loop(O, traj, start, base_row, truth, plan_row_=None, map_=None, steps=PERIODS, vt=SP.VT, window=SP.WINDOW, weights=None):
    """speed_plan_ref.cpu_loop with a road profile: before every advance_road the plant's road row is compose_row(base_row, truth[i]) at the nearest
    sample i of the TRUE pose; with plan_row_ given the plan reads `map_` ([M,8]; v_cap = vt, planned on the truth).
    -> speed_plan_ref.cpu_loop's dict, plus road [steps,8] (the row the plant drove on in each period), stats [steps,4] (the grip bookkeeping after
    each period) and margin_min (the smallest nearest-sample
    margin of all periods [m^2])"""
    from oracle import waypoints as W, vehicle_sim as Vs
    import scenario as S
    p = O.params(8, weights if weights is not None else S.WEIGHTS)
    s = Vs.initial_state(1, traj[start, 4], traj[start, 5], traj[start, 3])
    s[0, 3] = vt
    plant, base_row = R.DEFAULT_ROW[None, :], np.asarray(base_row, dtype=np.float64)
    kappa = SP.curvature(traj, window)[0] if plan_row_ is not None else None
    u_prev, U_prev, have_warm = np.zeros(2), None, False
    cmds, states, status, v_plan = np.zeros((steps, 1, 2)), np.zeros((steps + 1, 1, 8)), [], np.full(steps, float(vt))
    roads, stats = np.zeros((steps, 8)), np.zeros((steps, 4))
    states[0] = s
    stat, near = np.zeros((1, 4)), np.zeros(1, dtype=bool)
    margin_min = np.inf
    for k in range(steps):
        x, y, psi, v = s[0, 0:4]
        d2 = (traj[:, 4] - x) ** 2 + (traj[:, 5] - y) ** 2
        i = int(np.argmin(d2))
        two = np.partition(d2, 1)[:2]
        margin_min = min(margin_min, float(two[1] - two[0]))
        if plan_row_ is not None:
            v_plan[k] = plan_one(traj, kappa, map_, x, y, vt, plan_row_, i=i)["v_plan"]
        xr, yr, pr, _stop, _ci = W.get_waypoints(traj, x, y, psi, v_plan[k], traj_horizon=8)
        q = O.problem(p, [x, y, psi, v], np.stack([xr, yr, pr], 1), v_plan[k], u_prev)
        r = O.solve_condensed(p, q, o=O.opts(warm=1) if have_warm else O.opts(), U0=U_prev)
        cmd = r["U"][0].copy()
        u_prev, U_prev, have_warm = cmd.copy(), r["U"].copy(), True
        cmds[k, 0] = cmd
        status.append(r["status"])
        roads[k] = compose_row(base_row, truth[i])
        s, stat = RR.advance_road(s, cmds, k, plant, roads[k][None, :], [0], 2, SP.N_UPD, stat=stat, near=near)
        states[k + 1], stats[k] = s, stat[0]
    ect, _ = S.cross_track(traj[:, 4:6], states[:, 0, 0], states[:, 0, 1])
    return dict(state=states[:, 0], cmd=cmds[:, 0], status=np.array(status), stat=stat[0], stats=stats, near=bool(near[0]), ect=ect, v_plan=v_plan, road=roads,
                margin_min=margin_min, margin_low=bool(margin_min < SP.MARGIN))


def cached_loop(O, name):
    """arm `name` of arms(), computed once per process -> (cpu_loop's dict, trajectory, start index)"""
    _, _, _, tr, i0 = SP.loop_start()
    key = ("loop", name)
    if key not in _cache:
        a = arms()[name]
        _cache[key] = cpu_loop(O, tr, i0, a["base"], a["truth"], a["plan_row"], a["map"], steps=a["steps"], vt=a["vt"])
    return _cache[key], tr, i0
