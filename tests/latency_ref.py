"""TEST INFRASTRUCTURE: numpy restatement of the latency stages (kmpc_sim_advance_queue, kmpc_sense_delayed_batch, kmpc_cmd_in_force_batch,
kmpc_predict_ahead_batch), written from the text of include/kmpc.h, not from the kernels, and a CPU closed loop with all of them.

Where the device code keeps rings, the restatement keeps the WHOLE log -- cmds [P,B,2] with cmds[j] the command of period j, states [P,B,8] -- and
indexes it by period; a negative period is the command (0, 0).  The plant is plant_ref.update_plant and the Euler step estimator_ref.model_step:
both are restatements of their own headers' text.
"""
import numpy as np

import estimator_ref as E
import plant_ref as R

H = 0.01   # one update [s]


def in_force_period(tau, d, n):
    """j(tau, d) = floor((tau - d) / n), floor towards -infinity (numpy's // on integers)"""
    return (np.asarray(tau, dtype=np.int64) - np.asarray(d, dtype=np.int64)) // int(n)


def command_of(cmds, j):
    """cmds [P,B,2], j [B] periods -> [B,2]: vehicle b's command of period j[b], (0, 0) where j[b] < 0"""
    cmds = np.asarray(cmds, dtype=np.float64)
    j = np.asarray(j, dtype=np.int64)
    B = len(j)
    out = np.zeros((B, 2))
    ok = j >= 0
    if ok.any():
        out[ok] = cmds[j[ok], np.arange(B)[ok]]
    return out


def queue_split(cmd_delay, depth, n):
    """-> (q, r) of the clamped delay d = q n + r"""
    d = np.clip(np.asarray(cmd_delay, dtype=np.int64), 0, (depth - 1) * n)
    return d // n, d % n


def advance_queue(state, cmds, period, plant, cmd_delay, depth, n):
    """one call of kmpc_sim_advance_queue in period `period`, cmds[period] being this call's command -> state [B,8]: update `up` runs towards the
    command of period - q - (up < r), i.e. the plant of kmpc_sim_advance_plant with cmd = period - q's, cmd_held = period - q - 1's, delay r"""
    q, r = queue_split(cmd_delay, depth, n)
    new, _ = R.update_plant(state, command_of(cmds, period - q), plant, n_updates=n, cmd_delay=r, cmd_held=command_of(cmds, period - q - 1))
    return new


def sense_delayed(states, sensor, seed, period, meas_delay, depth, id_base=0):
    """states [P,B,8] (states[j]: the truth at period j) -> est [B,4]: the truth of period - L with this period's noise"""
    states = np.asarray(states, dtype=np.float64)
    B = states.shape[1]
    L = np.clip(np.asarray(meas_delay, dtype=np.int64), 0, min(depth - 1, period))
    return R.sense(states[period - L, np.arange(B)], sensor, seed, period, id_base=id_base)


def clamp_delays(period, cmd_delay, meas_delay, max_cmd_delay, max_meas_delay):
    d = np.clip(np.asarray(cmd_delay, dtype=np.int64), 0, max_cmd_delay)
    Lm = np.clip(np.asarray(meas_delay, dtype=np.int64), 0, min(max_meas_delay, period))
    return d, Lm


def cmd_in_force(cmds, period, n, cmd_delay, meas_delay, max_cmd_delay, max_meas_delay):
    """-> u [B,2]: the command in force at the midpoint of the period before the measurement's moment"""
    d, Lm = clamp_delays(period, cmd_delay, meas_delay, max_cmd_delay, max_meas_delay)
    tau = (period - Lm - 1) * n + n // 2
    return command_of(cmds, in_force_period(tau, d, n))


def predict_ahead(z, cmds, period, n, cmd_delay, meas_delay, max_cmd_delay, max_meas_delay, L_a=E.L_A, L_b=E.L_B):
    """z [B,4] valid at update (period - Lm) n -> z [B,4] at update period n + d: Lm n + d Euler steps of h = 0.01 s, each under the command in
    force at its update.  A vehicle that has no step left keeps its words untouched (zero delays: z bit for bit)."""
    z = np.array(z, dtype=np.float64, copy=True)
    d, Lm = clamp_delays(period, cmd_delay, meas_delay, max_cmd_delay, max_meas_delay)
    tau0, steps = (period - Lm) * n, Lm * n + d
    for k in range(int(steps.max()) if len(steps) else 0):
        active = k < steps
        u = command_of(cmds, np.where(active, in_force_period(tau0 + k, d, n), -1))   # a vehicle that is done reads no log
        with np.errstate(all="ignore"):
            new, _ = E.model_step(z, u, H, L_a, L_b)
        z = np.where(active[:, None], new, z)
    return z


def timeline(cmds, d, n, total):
    """brute force: the plant's input register starts at (0, 0); the command of period j is sent at update j n and delivered d updates later
    -> for one vehicle, the index of the period whose command is in the register at each update 0 ... total - 1 (-1: none yet)"""
    reg, out = -1, []
    in_flight = []
    for tau in range(total):
        if tau % n == 0 and tau // n < cmds:
            in_flight.append((tau + d, tau // n))
        for due, j in list(in_flight):
            if due == tau:
                reg = j
                in_flight.remove((due, j))
        out.append(reg)
    return np.array(out)


# ---------------------------------------------------------------- the loop setting shared by tests/test_latency.py's tests 6 and 7
VT, CMD_DELAY, MEAS_DELAY, N_UPD = 6.0, 25, 1, 10
Q_DEPTH = 4          # (4 - 1) * 10 >= 25
EST_Q, EST_R = (0.02, 0.02, 0.01, 0.1), (1e-3, 1e-3, 1e-4, 1e-3)    # Estimator's default q; r = Estimator.from_sensor's floor (no noise)


def cpu_loop(O, traj, X0, Y0, Psi0, steps, compensate=True, weights=None):
    """ONE vehicle on the CPU: plant with a command queue (true delay CMD_DELAY updates) -> stale fix (age MEAS_DELAY periods, no noise) ->
    estimator fed the logged command in force (estimator_input="history") -> predict-ahead -> waypoints -> solve (the oracle's condensed solver,
    warm-started) -> command log -> plant.  compensate=False: the same plant and sensor, the estimator fed the plant's actuator states
    (estimator_input="actuator", the loops' default) and no prediction.
    -> dict of per-step arrays: state [steps+1,8], cmd [steps,2], est, est_filt, est_pred [steps,4], status [steps]"""
    from oracle import waypoints as W, vehicle_sim as V
    import scenario as S
    p = O.params(8, weights if weights is not None else S.WEIGHTS)
    s = V.initial_state(1, X0, Y0, Psi0)
    s[0, 3] = VT
    row = np.zeros((1, 8))
    par = np.array([EST_Q + EST_R])
    plant = R.DEFAULT_ROW[None, :]
    rec = np.zeros((1, 16))
    u_prev, U_prev, have_warm, command_stop = np.zeros(2), None, False, False
    cmds, states = np.zeros((steps, 1, 2)), np.zeros((steps + 1, 1, 8))
    states[0] = s
    log = dict(cmd=[], est=[], est_filt=[], est_pred=[], status=[])
    for k in range(steps):
        z = sense_delayed(states, row, 0, k, [MEAS_DELAY], MEAS_DELAY + 1)
        if compensate:
            u = cmd_in_force(cmds, k, N_UPD, [CMD_DELAY], [MEAS_DELAY], CMD_DELAY, MEAS_DELAY)
        else:
            u = s[:, 6:8]
        rec, filt, _, _ = E.estimate(rec, z, u, par, dt=0.1)
        seen = predict_ahead(filt, cmds, k, N_UPD, [CMD_DELAY], [MEAS_DELAY], CMD_DELAY, MEAS_DELAY) if compensate else filt
        x, y, psi, v = seen[0]
        xr, yr, pr, stop, _ci = W.get_waypoints(traj, x, y, psi, VT, traj_horizon=8)
        command_stop = command_stop or stop
        assert not command_stop
        q = O.problem(p, [x, y, psi, v], np.stack([xr, yr, pr], 1), VT, u_prev)
        r = O.solve_condensed(p, q, o=O.opts(warm=1) if have_warm else O.opts(), U0=U_prev)
        cmd = r["U"][0].copy()
        u_prev, U_prev, have_warm = cmd.copy(), r["U"].copy(), True
        cmds[k, 0] = cmd
        log["status"].append(r["status"]); log["cmd"].append(cmd); log["est"].append(z[0].copy()); log["est_filt"].append(filt[0].copy())
        log["est_pred"].append(seen[0].copy())
        s = advance_queue(s, cmds, k, plant, [CMD_DELAY], Q_DEPTH, N_UPD)
        states[k + 1] = s
    out = {n: np.array(v) for n, v in log.items()}
    out["state"] = states[:, 0]
    return out


def starts(nv):
    """nv starts on path1, evenly from 5 % to 45 % along it, in turn 0.5 m left of it / 0.5 m right / on it with the heading off by +0.05 / -0.05 / 0
    rad, already at the target speed -> X0, Y0, Psi0 [nv], the oracle's trajectory table"""
    from oracle import waypoints as W
    import scenario as S
    arr, lat0, lon0 = S.path_arrays("path1_decimated.npz")
    tr = W.build_trajectory(arr["t"], arr["lat"], arr["lon"], arr["psi"], lat0, lon0)
    idx = (np.linspace(0.05, 0.45, nv) * len(tr)).astype(int)
    lat, dpsi = np.array([0.5, -0.5, 0.0])[np.arange(nv) % 3], np.array([0.05, -0.05, 0.0])[np.arange(nv) % 3]
    psi0 = tr[idx, 3]
    return tr[idx, 4] - lat * np.sin(psi0), tr[idx, 5] + lat * np.cos(psi0), psi0 + dpsi, tr


def rms_ect(traj, state):
    """rms cross-track error of one vehicle's states [K,8] against the path's polyline [m]"""
    import scenario as S
    e, _ = S.cross_track(traj[:, 4:6], state[:, 0], state[:, 1])
    return float(np.sqrt((e ** 2).mean()))
