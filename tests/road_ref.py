"""TEST INFRASTRUCTURE: numpy restatement of the plant with a road row per vehicle (kmpc_sim_advance_road), written from the text of include/kmpc.h,
not from the kernel, and the CPU closed loop that tests/test_road_ref.py and tests/test_road.py share.

update_road is plant_ref.update_plant's shape with the header's changes: dfe = df + DF_OFFSET in the tyre model, acce = ACC_GAIN * acc in vx's
derivative, each axle's force clipped by compare-and-select at mu x its static load, the two specific forces added in statements of their own.  The
queue is latency_ref's (queue_split / command_of): the whole command log, indexed by period.
"""
import numpy as np

import latency_ref as LR
import plant_ref as R
from oracle import vehicle_sim as V

FIELDS = ("mu_f", "mu_r", "a_long", "a_lat", "df_offset", "acc_gain")
NEUTRAL_ROW = np.array([np.inf, np.inf, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0])
G = 9.81
NEAR = 1e-9     # a force whose |F| / lim came this close to 1 may be counted as clipped on one side and not on the other


def rows(B, **kw):
    """[B,8] road rows: neutral, with `mu` (both axles) or any of FIELDS a scalar or one value per vehicle"""
    r = np.tile(NEUTRAL_ROW, (B, 1))
    for k, v in kw.items():
        for w in ((0, 1) if k == "mu" else (FIELDS.index(k),)):
            r[:, w] = v
    return r


def clip(x, lim):
    """x > lim ? lim : (x < -lim ? -lim : x): x's own bits inside the limit, a NaN passes"""
    with np.errstate(invalid="ignore"):
        return np.where(x > lim, lim, np.where(x < -lim, -lim, x))


def update_road(state, cmd, plant, road, n_updates=1, cmd_delay=None, cmd_held=None, stat=None, disc_steps=V.DISC_STEPS, near=None):
    """-> (state [B,8], stat [B,4]).  cmd / cmd_held / cmd_delay as plant_ref.update_plant's; stat [B,4] or None (zeros) is accumulated into a copy;
    near: a bool array [B] that is OR-ed with "some sub-step's |F| / lim came within NEAR of 1" (either axle)"""
    s = np.array(state, dtype=np.float64, copy=True)
    B = len(s)
    X, Y, psi, vx, vy, wz, acc, df = (s[:, i].copy() for i in range(8))
    cmd = np.asarray(cmd, dtype=np.float64)
    lf, lr, m, Iz, Cf, Cr, k_acc, k_df = (np.asarray(plant, dtype=np.float64)[:, i] for i in range(8))
    mu_f, mu_r, a_long, a_lat, df_offset, acc_gain = (np.asarray(road, dtype=np.float64)[:, i] for i in range(6))
    inv_m, inv_Iz = 1.0 / m, 1.0 / Iz
    with np.errstate(all="ignore"):
        lim_f = mu_f * (m * G * lr / (lf + lr))
        lim_r = mu_r * (m * G * lf / (lf + lr))
    d = np.zeros(B, dtype=np.int64) if cmd_delay is None else np.clip(np.asarray(cmd_delay, dtype=np.int64), 0, n_updates)
    held = cmd if cmd_held is None else np.asarray(cmd_held, dtype=np.float64)
    deltaT = V.DT_MODEL / disc_steps
    sat_f, sat_r = np.zeros(B), np.zeros(B)
    peak_f, peak_r = np.zeros(B), np.zeros(B)
    with np.errstate(all="ignore"):
        for it in range(n_updates * disc_steps):
            old = it < d * disc_steps
            acc_des, df_des = np.where(old, held[:, 0], cmd[:, 0]), np.where(old, held[:, 1], cmd[:, 1])
            moving = np.fabs(vx) > 1e-6
            dfe = df + df_offset
            acce = acc_gain * acc
            alpha_f = np.where(moving, dfe - np.arctan2(vy + lf * wz, vx), 0.0)
            alpha_r = np.where(moving, -np.arctan2(vy - lf * wz, vx), 0.0)          # lf, as in the reference
            Ff = Cf * alpha_f
            Fr = Cr * alpha_r
            Fyf, Fyr = clip(Ff, lim_f), clip(Fr, lim_r)
            sat_f += (Ff > lim_f) | (Ff < -lim_f)
            sat_r += (Fr > lim_r) | (Fr < -lim_r)
            peak_f = np.where(np.fabs(Ff) > peak_f, np.fabs(Ff), peak_f)
            peak_r = np.where(np.fabs(Fr) > peak_r, np.fabs(Fr), peak_r)
            if near is not None:
                near |= (np.fabs(np.fabs(Ff) / lim_f - 1.0) <= NEAR) | (np.fabs(np.fabs(Fr) / lim_r - 1.0) <= NEAR)
            vx0 = vx + deltaT * (acce + wz * vy)                                    # no Fyf sin(df) / m term, as in the reference
            vx_n = np.maximum(0.0, vx0 + deltaT * a_long)
            fwd = vx_n > 1e-6
            vy0 = vy + deltaT * (inv_m * (Fyf * np.cos(dfe) + Fyr) - wz * vx)
            vy_c = vy0 + deltaT * a_lat
            wz_c = wz + deltaT * (inv_Iz * (lf * Fyf * np.cos(dfe) - lr * Fyr))
            vy_n, wz_n = np.where(fwd, vy_c, 0.0), np.where(fwd, wz_c, 0.0)
            psi_n = psi + deltaT * wz
            X_n = X + deltaT * (vx * np.cos(psi) - vy * np.sin(psi))
            Y_n = Y + deltaT * (vx * np.sin(psi) + vy * np.cos(psi))
            X, Y = X_n, Y_n
            psi = (psi_n + np.pi) % (2.0 * np.pi) - np.pi
            vx, vy, wz = vx_n, vy_n, wz_n
            acc = k_acc * (acc_des - acc) * deltaT + acc
            df = k_df * (df_des - df) * deltaT + df
        out = np.zeros((B, 4)) if stat is None else np.array(stat, dtype=np.float64, copy=True)
        u_f, u_r = peak_f / lim_f, peak_r / lim_r
        out[:, 0] += sat_f
        out[:, 1] += sat_r
        out[:, 2] = np.where(u_f > out[:, 2], u_f, out[:, 2])
        out[:, 3] = np.where(u_r > out[:, 3], u_r, out[:, 3])
    return np.stack([X, Y, psi, vx, vy, wz, acc, df], axis=1), out


def advance_road(state, cmds, period, plant, road, cmd_delay, depth, n, stat=None, near=None):
    """one call of kmpc_sim_advance_road in period `period`, cmds[period] being this call's command -> (state [B,8], stat [B,4])"""
    q, r = LR.queue_split(cmd_delay, depth, n)
    return update_road(state, LR.command_of(cmds, period - q), plant, road, n_updates=n, cmd_delay=r, cmd_held=LR.command_of(cmds, period - q - 1),
                       stat=stat, near=near)


# ---------------------------------------------------------------- the random-rows case shared by the CPU and the GPU test
ROWS_SEED = 41


def random_rows(B=R.SPREAD_B, seed=ROWS_SEED):
    """seeded road rows: mu per axle independently +inf (half) or U(0.2, 1.2), A_LONG U(-1, 1), A_LAT U(-2, 2), DF_OFFSET U(-0.05, 0.05),
    ACC_GAIN U(0.7, 1.3)"""
    rng = np.random.default_rng(seed)
    r = np.tile(NEUTRAL_ROW, (B, 1))
    for w in (0, 1):
        r[:, w] = np.where(rng.random(B) < 0.5, np.inf, rng.uniform(0.2, 1.2, B))
    r[:, 2], r[:, 3] = rng.uniform(-1, 1, B), rng.uniform(-2, 2, B)
    r[:, 4], r[:, 5] = rng.uniform(-0.05, 0.05, B), rng.uniform(0.7, 1.3, B)
    return r


# ---------------------------------------------------------------- the closed loop of the issue's table
VT, N_UPD, PATH, AT, PERIODS = 6.0, 10, "path3_decimated.npz", 0.58, 120
LOOP_ROADS = (dict(), dict(mu=0.5), dict(mu=0.35))     # neutral, mu = 0.5, mu = 0.35


def loop_start(offsets=(0.0,)):
    """the path's point at AT of its length (by index) and its heading, shifted `offsets` m to the left -> X0, Y0, Psi0 [len(offsets)], trajectory"""
    from oracle import waypoints as W
    import scenario as S
    arr, lat0, lon0 = S.path_arrays(PATH)
    tr = W.build_trajectory(arr["t"], arr["lat"], arr["lon"], arr["psi"], lat0, lon0)
    i = int(AT * len(tr))
    off = np.asarray(offsets, dtype=np.float64)
    psi0 = np.full(len(off), tr[i, 3])
    return tr[i, 4] - off * np.sin(psi0), tr[i, 5] + off * np.cos(psi0), psi0, tr


def cpu_loop(O, traj, X0, Y0, Psi0, road_row, steps=PERIODS, weights=None):
    """ONE vehicle on the CPU, started at (X0, Y0, Psi0) already at VT: truth -> waypoints -> solve (the oracle's condensed solver at N = 8, the node's
    weights, warm-started; no stop latch) -> plant with the road row (queue of depth 2, no delay).
    -> dict: state [steps+1,8], cmd [steps,2], status [steps], stat [4], near (bool), ect [steps+1]"""
    from oracle import waypoints as W, vehicle_sim as Vs
    import scenario as S
    p = O.params(8, weights if weights is not None else S.WEIGHTS)
    s = Vs.initial_state(1, X0, Y0, Psi0)
    s[0, 3] = VT
    plant, road = R.DEFAULT_ROW[None, :], np.asarray(road_row, dtype=np.float64)[None, :]
    u_prev, U_prev, have_warm = np.zeros(2), None, False
    cmds, states, status = np.zeros((steps, 1, 2)), np.zeros((steps + 1, 1, 8)), []
    states[0] = s
    stat, near = np.zeros((1, 4)), np.zeros(1, dtype=bool)
    for k in range(steps):
        x, y, psi, v = s[0, 0:4]
        xr, yr, pr, _stop, _ci = W.get_waypoints(traj, x, y, psi, VT, traj_horizon=8)
        q = O.problem(p, [x, y, psi, v], np.stack([xr, yr, pr], 1), VT, u_prev)
        r = O.solve_condensed(p, q, o=O.opts(warm=1) if have_warm else O.opts(), U0=U_prev)
        cmd = r["U"][0].copy()
        u_prev, U_prev, have_warm = cmd.copy(), r["U"].copy(), True
        cmds[k, 0] = cmd
        status.append(r["status"])
        s, stat = advance_road(s, cmds, k, plant, road, [0], 2, N_UPD, stat=stat, near=near)
        states[k + 1] = s
    ect, _ = S.cross_track(traj[:, 4:6], states[:, 0, 0], states[:, 0, 1])
    return dict(state=states[:, 0], cmd=cmds[:, 0], status=np.array(status), stat=stat[0], near=bool(near[0]), ect=ect)


_LOOPS = {}


def cpu_loops(O, offsets=(0.0,)):
    """the three roads x the lateral offsets, computed once per process -> {(road index, offset): cpu_loop's dict}, trajectory"""
    key = tuple(offsets)
    if key not in _LOOPS:
        X0, Y0, P0, tr = loop_start(offsets)
        _LOOPS[key] = ({(ri, off): cpu_loop(O, tr, X0[oi], Y0[oi], P0[oi], rows(1, **kw)[0])
                        for ri, kw in enumerate(LOOP_ROADS) for oi, off in enumerate(offsets)}, tr)
    return _LOOPS[key]
