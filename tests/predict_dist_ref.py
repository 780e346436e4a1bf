"""TEST INFRASTRUCTURE: numpy restatement of the prediction ahead under estimated disturbances (kmpc_predict_ahead_dist_batch), written from the
text of include/kmpc.h, not from the kernel, on observer_ref.model_step (the observer's augmented Euler step) and latency_ref.clamp_delays /
in_force_period / command_of (the delay rules and the log lookup of kmpc_predict_ahead_batch).  As in latency_ref the restatement keeps the WHOLE
command log, cmds [P,B,2], where the device keeps a ring; ring_of() cuts the ring a call in a given period sees.

Also here: the seeded case the CPU and the GPU tests share, and a CPU closed loop with dead time AND a disturbed road in it: observer_ref.cpu_loop's
shape with latency_ref.sense_delayed, cmd_in_force and road_ref.advance_road behind a command queue.
"""
import numpy as np

import estimator_ref as E
import latency_ref as LR
import observer_ref as OR
import road_ref as RR

H = LR.H


def predict_ahead_dist(rec, est, cmds, period, n, cmd_delay, meas_delay, max_cmd_delay, max_meas_delay, L_a=OR.L_A, L_b=OR.L_B, psi_cap=OR.PSI_CAP):
    """rec [B,40] the observer's records, est [B,4] its est_out, cmds [P,B,2] -> z [B,4] at update period n + d: Lm n + d Euler steps of the
    augmented model from words 0 ... 6 of a live record, the heading shifted by clip(dpsi, psi_cap) at the end; a fresh record returns est"""
    rec, est = np.asarray(rec, dtype=np.float64), np.asarray(est, dtype=np.float64)
    xh = np.array(rec[:, 0:7], dtype=np.float64, copy=True)
    live = rec[:, OR.COUNT] != 0.0
    d, Lm = LR.clamp_delays(period, cmd_delay, meas_delay, max_cmd_delay, max_meas_delay)
    tau0, steps = (period - Lm) * n, Lm * n + d
    for k in range(int(steps.max()) if len(steps) else 0):
        active = k < steps
        u = LR.command_of(cmds, np.where(active, LR.in_force_period(tau0 + k, d, n), -1))   # a vehicle that is done reads no log
        with np.errstate(all="ignore"):
            new, _ = OR.model_step(xh, u, H, L_a, L_b)
        xh = np.where(active[:, None], new, xh)
    with np.errstate(all="ignore"):
        out = np.stack([xh[:, 0], xh[:, 1], OR.wrap(xh[:, 2] + OR.clip(xh[:, 4], psi_cap)), xh[:, 3]], axis=1)
    return np.where(live[:, None], out, est)


def ring_of(cmds, period, depth):
    """cmds [P,B,2] -> the ring [depth,B,2] a call in `period` sees: slot j mod depth holds period j's command for j = period - depth ... period - 1;
    slots of periods < 0 hold a number nobody may read (7.0)"""
    cmds = np.asarray(cmds, dtype=np.float64)
    ring = np.full((depth,) + cmds.shape[1:], 7.0)
    for j in range(max(period - depth, 0), period):
        ring[j % depth] = cmds[j]
    return ring


# ---------------------------------------------------------------- the seeded case shared by tests/test_predict_dist_ref.py (CPU) and tests/test_predict_dist.py (GPU)
SEED, B_CASE, N_UPD, DEPTH, MAX_CMD, MAX_MEAS = 67, 300, 10, 7, 35, 2
PERIODS = (0, 1, 2, 9)
N_LOG = 10                       # periods 0 ... 9 of the command log
FRESH = slice(0, 20)             # fresh records (word 35 == 0)
BEYOND = slice(20, 60)           # |dpsi| beyond psi_cap, both signs
SLOW = slice(60, 90)             # v near 0 and a braking command: the floor acts
SEAM = slice(90, 110)            # psi next to +-pi: the wrap acts


def seeded_case():
    """300 vehicles (two 256-thread blocks, the second a partial wave): cmd delays 0 ... 35 updates and meas delays 0 ... 2 periods per vehicle,
    depth 7 = 2 + ceil(35 / 10) + 1, n = 10, records in mid-run with disturbances of both signs, and the groups named above.
    -> dict(rec [B,40], est [B,4], cmds [10,B,2], cmd_delay [B], meas_delay [B], psi_cap)"""
    rng = np.random.default_rng(SEED)
    B = B_CASE
    rec = np.zeros((B, OR.WORDS))
    rec[:, 0:2] = rng.uniform(-500, 500, (B, 2))
    rec[:, 2] = rng.uniform(-np.pi, np.pi, B)
    rec[:, 3] = rng.uniform(2, 20, B)
    rec[:, 4:7] = rng.uniform(-1, 1, (B, 3)) * np.array([0.15, 0.05, 0.8])
    rec[BEYOND, 4] = np.where(np.arange(40) % 2 == 0, 1.0, -1.0) * rng.uniform(0.25, 0.4, 40)
    rec[SLOW, 3] = rng.uniform(0.0, 0.15, 30)
    rec[SLOW.start, 3] = 0.0
    rec[SEAM, 2] = np.where(np.arange(20) % 2 == 0, 1.0, -1.0) * (np.pi - rng.uniform(1e-6, 5e-3, 20))
    rec[:, 7:35] = OR.full_to_tri(OR.random_spd(rng, B))     # read by nobody: the prediction must not depend on them
    rec[:, OR.COUNT] = rng.integers(1, 500, B)
    rec[:, OR.SKIPPED] = rng.integers(0, 7, B)
    rec[FRESH] = 0.0
    est = np.stack([rng.uniform(-500, 500, B), rng.uniform(-500, 500, B), rng.uniform(-np.pi, np.pi, B), rng.uniform(0, 20, B)], 1)
    cmds = np.stack([rng.uniform(-1, 1, (N_LOG, B)), rng.uniform(-0.5, 0.5, (N_LOG, B))], axis=2)
    cmds[:, SLOW, 0] = -rng.uniform(0.5, 1.5, (N_LOG, 30)) - rec[SLOW, 6]        # acc + da < 0: v reaches the floor and stays
    cmd_delay = rng.integers(0, MAX_CMD + 1, B).astype(np.int32)
    meas_delay = rng.integers(0, MAX_MEAS + 1, B).astype(np.int32)
    cmd_delay[110:120], meas_delay[110:120] = 0, 0                               # no step at all: est_out's convention alone
    cmd_delay[120:124], meas_delay[120:124] = MAX_CMD, MAX_MEAS                  # the 55 steps of the bound
    cmd_delay[124], cmd_delay[125], meas_delay[126] = -3, 90, 7                  # clamped by the caps
    return dict(rec=rec, est=est, cmds=cmds, cmd_delay=cmd_delay, meas_delay=meas_delay, psi_cap=OR.PSI_CAP)


def case_reference(case=None):
    """{period: z_out [B,4]} of the restatement over PERIODS"""
    c = case if case is not None else seeded_case()
    return {p: predict_ahead_dist(c["rec"], c["est"], c["cmds"], p, N_UPD, c["cmd_delay"], c["meas_delay"], MAX_CMD, MAX_MEAS, psi_cap=c["psi_cap"])
            for p in PERIODS}


# ---------------------------------------------------------------- the closed loop of the issue's table
VT, PLANT_N = RR.VT, RR.N_UPD
CMD_DELAY, MEAS_DELAY = 25, 1             # 0.25 s + 0.1 s = 0.35 s of dead time
Q_SCALE = 0.25                            # the observer's q_dist against its default at that dead time
LOOP_STEPS, TAIL = 240, 180
ROADS = dict(neutral=dict(), bank_offset=dict(a_lat=1.5, df_offset=0.03), offset=dict(df_offset=0.06), grade=dict(a_long=-0.5))
MODES = ("estimator+compensator", "observer+plain", "observer+dist")
EST_Q, EST_R = LR.EST_Q, LR.EST_R         # latency_ref's: Estimator's default q, and the r of a noiseless fix (Estimator.from_sensor's floor)


def cpu_loop(O, traj, X0, Y0, Psi0, road_row, mode, steps=LOOP_STEPS, cmd_delay=CMD_DELAY, meas_delay=MEAS_DELAY, q_scale=Q_SCALE, obs=None):
    """ONE vehicle on the CPU, started at (X0, Y0, Psi0) already at VT: road plant behind a command queue (true delay `cmd_delay` updates) -> stale
    fix (age `meas_delay` periods, no noise) -> filter fed the logged command in force (estimator_input="history") -> prediction ahead ->
    waypoints -> solve (the oracle's condensed solver at N = 8, warm-started) -> command offset (observer modes) -> command log -> plant.
    The controller's assumed delays are the true ones.  mode:
      "estimator+compensator"  estimator_ref.estimate (EST_Q, EST_R) + latency_ref.predict_ahead
      "observer+plain"         observer_ref.observe + cmd_offset, and latency_ref.predict_ahead on the observer's est_out (the undisturbed model)
      "observer+dist"          observer_ref.observe + cmd_offset, and predict_ahead_dist on the observer's record
    The observer runs with DisturbanceObserver's defaults and q_dist x `q_scale` (or the keywords in `obs`).  The log holds the command as sent.
    -> dict: state [steps+1,8], cmd [steps,2] (as sent), status [steps], ect [steps+1], dist [steps,3], est, est_filt, est_pred [steps,4]"""
    from oracle import waypoints as W, vehicle_sim as Vs
    import plant_ref as R_
    import scenario as S
    assert mode in MODES
    o = dict(q=OR.Q, q_dist=tuple(q_scale * np.array(OR.Q_DIST)), r=OR.R, p0=OR.P0, v_min=OR.V_MIN, psi_cap=OR.PSI_CAP, acc_cap=OR.ACC_CAP,
             df_cap=OR.DF_CAP)
    o.update(obs or {})
    observer = mode != "estimator+compensator"
    p = O.params(8, S.WEIGHTS)
    s = Vs.initial_state(1, X0, Y0, Psi0)
    s[0, 3] = VT
    plant, road = R_.DEFAULT_ROW[None, :], np.asarray(road_row, dtype=np.float64)[None, :]
    sensor = np.zeros((1, 8))
    q_depth = -(-cmd_delay // PLANT_N) + 1                       # (depth - 1) n >= cmd_delay, at least 2
    q_depth = max(q_depth, 2)
    u_prev, U_prev, have_warm = np.zeros(2), None, False
    cmds, states, status = np.zeros((steps, 1, 2)), np.zeros((steps + 1, 1, 8)), []
    states[0] = s
    stat, near = np.zeros((1, 4)), np.zeros(1, dtype=bool)
    rec40, rec16 = np.zeros((1, OR.WORDS)), np.zeros((1, 16))
    par16, par8 = OR.param_rows(1, o["q"], o["q_dist"], o["r"], o["p0"]), np.array([tuple(EST_Q) + tuple(EST_R)])
    log = dict(dist=np.zeros((steps, 3)), est=np.zeros((steps, 4)), est_filt=np.zeros((steps, 4)), est_pred=np.zeros((steps, 4)))
    dl = ([cmd_delay], [meas_delay], cmd_delay, meas_delay)
    for k in range(steps):
        z = LR.sense_delayed(states, sensor, 0, k, [meas_delay], meas_delay + 1)
        u = LR.cmd_in_force(cmds, k, PLANT_N, *dl)
        if observer:
            rec40, filt, log["dist"][k:k + 1], _, _ = OR.observe(rec40, z, u, par16, dt=0.1, v_min=o["v_min"], psi_cap=o["psi_cap"])
        else:
            rec16, filt, _, _ = E.estimate(rec16, z, u, par8, dt=0.1)
        if mode == "observer+dist":
            seen = predict_ahead_dist(rec40, filt, cmds, k, PLANT_N, *dl, psi_cap=o["psi_cap"])
        else:
            seen = LR.predict_ahead(filt, cmds, k, PLANT_N, *dl)
        log["est"][k], log["est_filt"][k], log["est_pred"][k] = z[0], filt[0], seen[0]
        x, y, psi, v = seen[0]
        xr, yr, pr, _stop, _ci = W.get_waypoints(traj, x, y, psi, VT, traj_horizon=8)
        q = O.problem(p, [x, y, psi, v], np.stack([xr, yr, pr], 1), VT, u_prev)
        r = O.solve_condensed(p, q, o=O.opts(warm=1) if have_warm else O.opts(), U0=U_prev)
        cmd = r["U"][0].copy()
        u_prev, U_prev, have_warm = cmd.copy(), r["U"].copy(), True
        if observer:
            cmd = OR.cmd_offset(rec40, None, o["acc_cap"], o["df_cap"], cmd[None, :])[0]
        cmds[k, 0] = cmd
        status.append(r["status"])
        s, stat = RR.advance_road(s, cmds, k, plant, road, [cmd_delay], q_depth, PLANT_N, stat=stat, near=near)
        states[k + 1] = s
    ect, _ = S.cross_track(traj[:, 4:6], states[:, 0, 0], states[:, 0, 1])
    out = dict(state=states[:, 0], cmd=cmds[:, 0], status=np.array(status), ect=ect)
    out.update(log)
    return out


_LOOPS = {}


def cpu_loops(O, road, modes=MODES, offset=0.0, **kw):
    """ROADS[road] x modes from the start `offset` m left of the path, computed once per process -> {mode: cpu_loop's dict}, trajectory"""
    X0, Y0, P0_, tr = RR.loop_start((offset,))
    out = {}
    for mode in modes:
        key = (road, mode, offset, tuple(sorted(kw.items())))
        if key not in _LOOPS:
            _LOOPS[key] = cpu_loop(O, tr, X0[0], Y0[0], P0_[0], RR.rows(1, **ROADS[road])[0], mode, **kw)
        out[mode] = _LOOPS[key]
    return out, tr


def tail_mean(run, steps=LOOP_STEPS):
    """|mean e_ct| over periods TAIL ... steps [m]"""
    return float(abs(run["ect"][TAIL:steps + 1].mean()))
