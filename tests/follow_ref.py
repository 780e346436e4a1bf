"""TEST INFRASTRUCTURE: numpy restatement of car following (kmpc_follow_fleet), written from the text of include/kmpc_follow.h, not from the kernel:
the O(B^2) leader search as one masked argmin per follower, the law operation by operation, the running record; the seeded draw that
tests/test_follow_ref.py and tests/test_follow.py share; and a CPU platoon loop on the oracle's waypoints and solver, the track score's restated
arclength and road_ref's plant (speed_plan_ref.cpu_loop's shape, for B vehicles on one path that see each other).
"""
import numpy as np

import plant_ref as R
import road_ref as RR
import track_score_ref as TS

FIELDS = ("d_min", "t_headway", "a_brake", "k_gap", "length")
STAT_FIELDS = ("n", "n_leader", "n_bound", "n_contact", "min_gap", "max_closing")
DEFAULT_ROW = np.array([5.0, 1.0, 0.7, 0.5, 4.9, 0.0, 0.0, 0.0])


def rows(B, **kw):
    """[B,8] following rows: the default, with any of FIELDS a scalar or one value per vehicle"""
    r = np.tile(DEFAULT_ROW, (B, 1))
    for k, v in kw.items():
        r[:, FIELDS.index(k)] = v
    return r


def fresh_stat(B):
    st = np.zeros((B, 8))
    st[:, 4] = np.inf
    return st


def usable(s, v, path_id=None, present=None):
    ok = np.isfinite(s) & np.isfinite(v)
    if present is not None:
        ok &= np.asarray(present) != 0
    if path_id is not None:
        ok &= np.asarray(path_id) >= 0
    return ok


def leaders(s, v, path_id=None, present=None):
    """-> leader [B] (int, -1 = none), diff [B] (s_leader - s_b as one rounded subtraction; +inf without a leader)"""
    s, v = np.asarray(s, dtype=np.float64), np.asarray(v, dtype=np.float64)
    B = len(s)
    pid = np.zeros(B, dtype=np.int64) if path_id is None else np.asarray(path_id, dtype=np.int64)
    ok = usable(s, v, path_id, present)
    idx = np.arange(B)
    leader, diff = np.full(B, -1, dtype=np.int64), np.full(B, np.inf)
    for b in range(B):
        if not ok[b]:
            continue
        with np.errstate(all="ignore"):
            ahead = (s > s[b]) | ((s == s[b]) & (idx < b))
            d = np.where(ok & (pid == pid[b]) & ahead, s - s[b], np.inf)
        j = int(np.argmin(d))            # first occurrence: the lowest j among equal differences
        if d[j] < np.inf:
            leader[b], diff[b] = j, d[j]
    return leader, diff


def law(diff, v_b, v_j, row, v_cap):
    """the law for followers WITH a leader, arrays throughout; row [n,8] -> dict gap, v_f, v_out, bound, v_safe, v_gap, rad"""
    d_min, t_h, a_b, k_gap, length = (row[:, i] for i in range(5))
    with np.errstate(all="ignore"):
        gap = diff - length
        g = gap - d_min
        gp = np.where(g > 0.0, g, 0.0)
        at = a_b * t_h
        rad = (at * at + v_j * v_j) + (2.0 * a_b) * gp
        v_safe = np.sqrt(rad) - at
        v_gap = v_j + k_gap * (g - t_h * v_b)
        v_f = np.where(v_gap < v_safe, v_gap, v_safe)
        v_f = np.where(v_f > 0.0, v_f, 0.0)
        bound = v_f < v_cap
    return dict(gap=gap, v_f=v_f, v_out=np.where(bound, v_f, v_cap), bound=bound, v_safe=v_safe, v_gap=v_gap, rad=rad, at=at)


def follow(s, v, path_id, present, rows_, v_cap, stat=None):
    """one call of kmpc_follow_fleet -> dict v_out [B], gap [B], v_lead [B], leader [B], bound [B], safe_arm [B] (the cap is the sqrt arm's value),
    stat [B,8] (a new array; `stat` None: a fresh record)"""
    s, v, v_cap = (np.asarray(a, dtype=np.float64) for a in (s, v, v_cap))
    B = len(s)
    leader, diff = leaders(s, v, path_id, present)
    has = leader >= 0
    v_out, gap, v_lead, bound, safe_arm = v_cap.copy(), np.full(B, np.inf), np.zeros(B), np.zeros(B, dtype=bool), np.zeros(B, dtype=bool)
    st = fresh_stat(B) if stat is None else np.array(stat, dtype=np.float64)
    st[:, 0] += 1.0
    if has.any():
        f = np.flatnonzero(has)
        vj = v[leader[f]]
        o = law(diff[f], v[f], vj, np.asarray(rows_, dtype=np.float64)[f], v_cap[f])
        v_out[f], gap[f], v_lead[f], bound[f] = o["v_out"], o["gap"], vj, o["bound"]
        with np.errstate(all="ignore"):
            safe_arm[f] = o["bound"] & ~(o["v_gap"] < o["v_safe"]) & (o["v_safe"] > 0.0)
            st[f, 1] += 1.0
            st[f, 2] += o["bound"]
            st[f, 3] += o["gap"] < 0.0
            st[f, 4] = np.where(o["gap"] < st[f, 4], o["gap"], st[f, 4])
            c = v[f] - vj
            st[f, 5] = np.where(c > st[f, 5], c, st[f, 5])
    return dict(v_out=v_out, gap=gap, v_lead=v_lead, leader=leader, bound=bound, safe_arm=safe_arm, stat=st)


# ---------------------------------------------------------------- the seeded draws shared by the CPU and the GPU tests
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 513, 1000, 1023, 1024, 1025, 2049)     # wave and tile edges: 64 followers per workgroup, 1024 candidates per tile


def draw(B, seed=0, paths=3, bad=True):
    """B vehicles: s a multiple of 0.5 m in [0, 200] (exact ties and equal differences occur), speed U(0, 10), v_cap U(2, 12), random rows (D_MIN
    U(0, 8), T U(0, 2), A_BRAKE U(0.3, 2), K_GAP U(0, 1), LENGTH U(3, 6), words 5 ... 7 junk), path ids in [0, paths) or None for paths == 0.
    With bad=True about 5 % of the vehicles have NaN or +-inf in s or speed, 10 % are not present and 5 % have path id -1.
    -> dict s, v, path_id (int32 or None), present (uint8), rows [B,8], v_cap"""
    rng = np.random.default_rng(1000 * B + seed)
    s = 0.5 * rng.integers(0, 401, B).astype(np.float64)
    v = rng.uniform(0.0, 10.0, B)
    pid = rng.integers(0, paths, B).astype(np.int32) if paths else None
    present = np.ones(B, dtype=np.uint8)
    r = np.tile(DEFAULT_ROW, (B, 1))
    r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4] = rng.uniform(0, 8, B), rng.uniform(0, 2, B), rng.uniform(0.3, 2, B), rng.uniform(0, 1, B), rng.uniform(3, 6, B)
    r[:, 5:8] = rng.uniform(-9, 9, (B, 3))
    v_cap = rng.uniform(2.0, 12.0, B)
    if bad:
        junk = np.array([np.nan, np.inf, -np.inf])
        hit = rng.random(B) < 0.05
        which = rng.random(B) < 0.5
        s[hit & which] = junk[rng.integers(0, 3, int((hit & which).sum()))]
        v[hit & ~which] = junk[rng.integers(0, 3, int((hit & ~which).sum()))]
        present[rng.random(B) < 0.10] = 0
        if pid is not None:
            pid[rng.random(B) < 0.05] = -1
    return dict(s=s, v=v, path_id=pid, present=present, rows=r, v_cap=v_cap)


# ---------------------------------------------------------------- the CPU platoon loop
N_UPD = 10
CASES = {   # the prototype's cases with three vehicles: vehicle 0 is the slow leader, in front; every vehicle starts on the path at its own target speed
    "path1": dict(path=0, spacing=20.0, targets=(3.0, 6.0, 6.0), row=dict()),
    "path2_T05": dict(path=1, spacing=12.0, targets=(3.0, 6.0, 6.0), row=dict(t_headway=0.5)),
}
S_FIRST = 5.0     # arclength of the last vehicle's start sample [m] (the first sample at or beyond it)


def platoon_start(traj, spacing, n):
    """sample indices of n vehicles, vehicle 0 in front: the first samples at or beyond S_FIRST + (n - 1 - b) * spacing"""
    s = traj[:, 6]
    return np.array([int(np.argmax(s >= S_FIRST + (n - 1 - b) * spacing)) for b in range(n)])


def cpu_platoon(O, traj, start, targets, rows_=None, steps=150, weights=None):
    """B vehicles on ONE path on the CPU, vehicle b started on the path at sample start[b], at its heading, already at targets[b].  Per period:
    the truth's arclengths (the track score's restatement) and speeds -> follow() with v_cap = targets -> per vehicle the oracle's waypoints and
    condensed solver at that speed (N = 8, the node's weights, warm-started; no stop latch) -> road_ref's plant on the neutral road (queue of depth
    2, no delay).  rows_ None: the stage only watches (v_follow = targets), so that the gaps of a fleet without it can be read.
    -> dict state [steps+1,B,8], cmd [steps,B,2], status [steps,B], v_follow [steps,B], gap [steps,B], leader [steps,B], stat [B,8], stop (bool: some
    period's waypoints ran off the path's end), final_gap [B] (of the last state)"""
    from oracle import waypoints as W, vehicle_sim as Vs
    import scenario as S
    B = len(start)
    targets = np.asarray(targets, dtype=np.float64)
    p = O.params(8, weights if weights is not None else S.WEIGHTS)
    s = np.concatenate([Vs.initial_state(1, traj[i, 4], traj[i, 5], traj[i, 3]) for i in start])
    s[:, 3] = targets
    plant, road = np.tile(R.DEFAULT_ROW, (B, 1)), np.tile(RR.NEUTRAL_ROW, (B, 1))
    watch = rows_ is None
    frows = rows(B) if watch else np.asarray(rows_, dtype=np.float64)
    u_prev, U_prev, have_warm = np.zeros((B, 2)), [None] * B, False
    cmds, states = np.zeros((steps, B, 2)), np.zeros((steps + 1, B, 8))
    status, v_follow, gap, leader = np.zeros((steps, B), dtype=np.int64), np.zeros((steps, B)), np.zeros((steps, B)), np.zeros((steps, B), dtype=np.int64)
    states[0] = s
    pstat, near, fstat, stop_any = np.zeros((B, 4)), np.zeros(B, dtype=bool), fresh_stat(B), False

    def see(state, stat):
        s_along = TS.errors(traj, state[:, 0], state[:, 1], state[:, 2])["s_along"]
        return follow(s_along, state[:, 3], None, None, frows, targets, stat)
    for k in range(steps):
        f = see(s, fstat)
        fstat = f["stat"]
        v_follow[k], gap[k], leader[k] = (targets if watch else f["v_out"]), f["gap"], f["leader"]
        for b in range(B):
            x, y, psi, v = s[b, 0:4]
            xr, yr, pr, stop, _ci = W.get_waypoints(traj, x, y, psi, v_follow[k, b], traj_horizon=8)
            stop_any |= bool(stop)
            q = O.problem(p, [x, y, psi, v], np.stack([xr, yr, pr], 1), v_follow[k, b], u_prev[b])
            r = O.solve_condensed(p, q, o=O.opts(warm=1) if have_warm else O.opts(), U0=U_prev[b])
            cmds[k, b] = r["U"][0]
            u_prev[b], U_prev[b] = r["U"][0].copy(), r["U"].copy()
            status[k, b] = r["status"]
        have_warm = True
        s, pstat = RR.advance_road(s, cmds, k, plant, road, [0] * B, 2, N_UPD, stat=pstat, near=near)
        states[k + 1] = s
    return dict(state=states, cmd=cmds, status=status, v_follow=v_follow, gap=gap, leader=leader, stat=fstat, stop=stop_any,
                final_gap=see(s, None)["gap"])


_cache = {}


def cached_platoon(O, case, with_stage=True, steps=150):
    """a case of CASES, with the stage or only watched, computed once per process -> (cpu_platoon's dict, trajectory, start indices)"""
    import fleet_scenario as F
    c = CASES[case]
    tr = F.trajectory(c["path"])
    start = platoon_start(tr, c["spacing"], len(c["targets"]))
    key = (case, with_stage, steps)
    if key not in _cache:
        _cache[key] = cpu_platoon(O, tr, start, c["targets"], rows(len(start), **c["row"]) if with_stage else None, steps=steps)
    return _cache[key], tr, start
