"""TEST INFRASTRUCTURE: numpy restatement of the measurement stage with sensor faults (kmpc_sense_faults_batch), written from the text of
include/kmpc.h, not from the kernel, on top of plant_ref.philox4x32_10 / plant_ref.sense and latency_ref.sense_delayed; the 300-vehicle case the
CPU and the GPU tests share; and a one-vehicle CPU closed loop with the stage in it (the oracle's waypoints and solver, the restated plant and
estimator).

Sources s = 0 GPS (x, y), 1 IMU (psi), 2 SPD (v).  Rows and records are [B,16] float64 in the header's word order.
"""
import numpy as np

import estimator_ref as E
import latency_ref as LR
import plant_ref as R

WORDS = 16
P_LOSE, P_REGAIN, WIN_FROM, WIN_LEN, P_OUTLIER, OUTLIER_SIGMA, MAX_AGE = 0, 3, 6, 9, 12, 13, 14      # KMPC_FAULT_*: first word of each group
HELD, COUNT, CHAIN, AGE, N_SILENT, LONGEST, N_OUTLIER = 0, 4, 5, 6, 9, 12, 15                         # KMPC_FAULTREC_*
F_SILENT, F_OUTLIER, F_BLIND, F_FRESH, F_RESET = (1, 2, 4), 8, 16, 32, 64                             # KMPC_FAULT_FLAG_*
NEUTRAL = np.array([0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, np.inf, 0], dtype=np.float64)
SOURCE_OF = (0, 0, 1, 2)       # channel x, y, psi, v -> its source


def fault_uniforms(seed, gid, period):
    """the four uniforms of the fault draw of vehicle `gid` in period `period`: the measurement draw's key, the counter's top bit set"""
    M = R.M32
    w = R.philox4x32_10((gid & M, (gid >> 32) & M, period & M, ((period >> 32) & M) ^ 0x80000000), (seed & M, (seed >> 32) & M))
    return (np.array(w, dtype=np.float64) + 0.5) * 2.0 ** -32


def decide(faults, rec, seed, period, id_base=0):
    """the decisions of one call, before any measurement -> dict(fresh, reset [B] bool, chain, silent [B,3] bool, outlier [B] bool)"""
    faults, rec = np.asarray(faults, dtype=np.float64), np.asarray(rec, dtype=np.float64)
    B = len(rec)
    count, chain_w = rec[:, COUNT], rec[:, CHAIN]
    with np.errstate(invalid="ignore"):
        reset = ~(np.isfinite(count) & (count >= 0.0)) | ~np.isin(chain_w, np.arange(8.0))
        fresh = reset | (count == 0.0)
        was = np.where(fresh, 0, np.where(np.isin(chain_w, np.arange(8.0)), chain_w, 0.0)).astype(np.int64)
        u = np.array([fault_uniforms(seed, id_base + b, period) for b in range(B)]).reshape(B, 4)
        p = float(period)
        chain, silent = np.zeros((B, 3), bool), np.zeros((B, 3), bool)
        for s in range(3):
            was_s = ((was >> s) & 1) == 1
            ch = np.where(was_s, ~(u[:, s] < faults[:, P_REGAIN + s]), u[:, s] < faults[:, P_LOSE + s])
            frm, ln = faults[:, WIN_FROM + s], faults[:, WIN_LEN + s]
            sched = (ln > 0.0) & (p >= frm) & (p < frm + ln)
            chain[:, s] = ~fresh & ch
            silent[:, s] = ~fresh & (ch | sched)
        outlier = ~fresh & ~silent[:, 0] & (u[:, 3] < faults[:, P_OUTLIER])
    return dict(fresh=fresh, reset=reset, chain=chain, silent=silent, outlier=outlier)


def effective_sensor(sensor, faults, outlier):
    """the vehicle's sensor row with SIGMA_X, SIGMA_Y replaced by OUTLIER_SIGMA where `outlier`"""
    sr = np.array(sensor, dtype=np.float64, copy=True)
    sr[outlier, 0] = np.asarray(faults)[outlier, OUTLIER_SIGMA]
    sr[outlier, 1] = np.asarray(faults)[outlier, OUTLIER_SIGMA]
    return sr


def apply(d, m, faults, rec):
    """decisions d and the measured values m [B,4] -> dict(rec, z, held [B,4], flags [B] int32, blind [B] uint8): selections and counts only"""
    faults = np.asarray(faults, dtype=np.float64)
    old = np.where(d["fresh"][:, None], 0.0, np.asarray(rec, dtype=np.float64))
    new = np.zeros_like(old)
    sil_c = d["silent"][:, SOURCE_OF]
    z = np.where(sil_c, np.nan, m)
    held = np.where(sil_c, old[:, HELD:HELD + 4], m)
    new[:, HELD:HELD + 4] = held
    sil = d["silent"]
    age = np.where(sil, old[:, AGE:AGE + 3] + 1.0, 0.0)
    new[:, AGE:AGE + 3] = age
    new[:, N_SILENT:N_SILENT + 3] = old[:, N_SILENT:N_SILENT + 3] + sil
    with np.errstate(invalid="ignore"):
        new[:, LONGEST:LONGEST + 3] = np.where(age > old[:, LONGEST:LONGEST + 3], age, old[:, LONGEST:LONGEST + 3])
        blind = (age > faults[:, MAX_AGE:MAX_AGE + 1]).any(1)
    new[:, N_OUTLIER] = old[:, N_OUTLIER] + d["outlier"]
    new[:, COUNT] = old[:, COUNT] + 1.0
    new[:, CHAIN] = (d["chain"] * np.array([1, 2, 4])).sum(1)
    flags = ((sil * np.array(F_SILENT)).sum(1) + F_OUTLIER * d["outlier"] + F_BLIND * blind + F_FRESH * d["fresh"] + F_RESET * d["reset"]).astype(np.int32)
    return dict(rec=new, z=z, held=held, flags=flags, blind=blind.astype(np.uint8))


def sense_faults(state, sensor, faults, rec, seed, period, id_base=0):
    """one call without a ring: state [B,>=4] is this period's truth -> apply()'s dict plus the decisions and `sensor_eff`"""
    d = decide(faults, rec, seed, period, id_base)
    sr = effective_sensor(sensor, faults, d["outlier"])
    with np.errstate(all="ignore"):
        m = R.sense(state, sr, seed, period, id_base=id_base)
    return dict(apply(d, m, faults, rec), sensor_eff=sr, measured=m, **d)


def sense_faults_delayed(states, sensor, faults, rec, seed, period, meas_delay, depth, id_base=0):
    """one call with a ring: states [P,B,8] is the log of truths (states[j]: period j's); the truth of period - L is measured, everything else
    belongs to `period`"""
    d = decide(faults, rec, seed, period, id_base)
    sr = effective_sensor(sensor, faults, d["outlier"])
    with np.errstate(all="ignore"):
        m = LR.sense_delayed(states, sr, seed, period, meas_delay, depth, id_base=id_base)
    return dict(apply(d, m, faults, rec), sensor_eff=sr, measured=m, **d)


# ---------------------------------------------------------------- the committed case shared by the CPU and the GPU tests
CASE_SEED, CASE_B, CASE_PERIODS, CASE_NOISE_SEED, CASE_ID_BASE = 41, 300, 40, 2 ** 63 + 29, 7
GROUPS = ("neutral", "chains", "windows", "outliers", "everything", "sticky")


def committed_case():
    """300 vehicles x 40 periods; the fault row of vehicle b belongs to group b % 6:
      0 neutral      1 random chains (P_LOSE 0.1 ... 0.4, P_REGAIN 0.2 ... 0.6 per source)      2 scheduled windows (from 1 ... 29, length 0 ... 14)
      3 outliers (P_OUTLIER 0.3 ... 0.7, OUTLIER_SIGMA 3 m)      4 everything, with MAX_AGE 0 ... 5      5 sticky (P_LOSE 0.1, P_REGAIN 0)
    states as plant_ref.draw_states draws them, anew every period; sensor rows with noise and bias, vehicles 60 ... 89 noiseless.
    -> dict(states [40,300,8], sensor [300,8], faults [300,16], seed, id_base)"""
    rng = np.random.default_rng(CASE_SEED)
    B, K = CASE_B, CASE_PERIODS
    states = np.stack([R.draw_states(rng, B)[0] for _ in range(K)])
    sensor = np.tile([0.2, 0.2, 0.01, 0.1, 0.05, -0.05, 0.001, 0.0], (B, 1))
    sensor[60:90, 0:4] = 0.0
    faults = np.tile(NEUTRAL, (B, 1))
    g = np.arange(B) % 6
    lose, regain = rng.uniform(0.1, 0.4, (B, 3)), rng.uniform(0.2, 0.6, (B, 3))
    frm, ln = rng.integers(1, 30, (B, 3)).astype(float), rng.integers(0, 15, (B, 3)).astype(float)
    pout = rng.uniform(0.3, 0.7, B)
    age = rng.integers(0, 6, B).astype(float)
    for grp in (1, 4):
        faults[g == grp, P_LOSE:P_LOSE + 3], faults[g == grp, P_REGAIN:P_REGAIN + 3] = lose[g == grp], regain[g == grp]
    for grp in (2, 4):
        faults[g == grp, WIN_FROM:WIN_FROM + 3], faults[g == grp, WIN_LEN:WIN_LEN + 3] = frm[g == grp], ln[g == grp]
    for grp in (3, 4):
        faults[g == grp, P_OUTLIER], faults[g == grp, OUTLIER_SIGMA] = pout[g == grp], 3.0
    faults[g == 4, MAX_AGE] = age[g == 4]
    faults[g == 5, P_LOSE:P_LOSE + 3], faults[g == 5, P_REGAIN:P_REGAIN + 3] = 0.1, 0.0
    return dict(states=states, sensor=sensor, faults=faults, seed=CASE_NOISE_SEED, id_base=CASE_ID_BASE, group=g)


def run_case(case, periods=None, faults=None):
    """the restatement over the case from fresh records -> dict of per-period arrays: rec [K,B,16], z, held, measured [K,B,4], flags [K,B],
    blind [K,B], silent, chain [K,B,3], outlier, fresh [K,B], sensor_eff [K,B,8]"""
    K = case["states"].shape[0] if periods is None else periods
    faults = case["faults"] if faults is None else faults
    rec = np.zeros((case["states"].shape[1], WORDS))
    log = {}
    for p in range(K):
        o = sense_faults(case["states"][p], case["sensor"], faults, rec, case["seed"], p, case["id_base"])
        rec = o["rec"]
        for k, v in o.items():
            log.setdefault(k, []).append(v)
    return {k: np.array(v) for k, v in log.items()}


# ---------------------------------------------------------------- one-vehicle CPU loops: path3, on the path at 6 m/s
VT, START, STEPS, N_UPD = 6.0, 0.56, 150, 10
WINDOW = (20, 30)            # GPS silent for periods 20 ... 49
EST_Q, EST_R = LR.EST_Q, LR.EST_R


def path3():
    """the oracle's trajectory table of path3 and the start on it -> (traj, X0, Y0, Psi0)"""
    from oracle import waypoints as W
    import scenario as S
    arr, lat0, lon0 = S.path_arrays("path3_decimated.npz")
    tr = W.build_trajectory(arr["t"], arr["lat"], arr["lon"], arr["psi"], lat0, lon0)
    i = int(START * len(tr))
    return tr, tr[i, 4], tr[i, 5], tr[i, 3]


def cpu_loop(O, traj, X0, Y0, Psi0, steps, fault_row, estimator=False, blind_stop=False, sensor_row=None, gate=0.0, seed=0, gid=0, weights=None):
    """ONE vehicle on the CPU: the reference's plant -> the measurement stage with faults (no ring) -> either the held state (estimator=False: what
    state_publisher.py publishes) or estimator_ref.estimate fed z and the plant's actuator states (estimator_input="actuator") -> waypoints ->
    solve (the oracle's condensed solver, warm-started) -> command stage, with `blind` OR-ed into the helper's stop flag when blind_stop -> plant.
    A latched vehicle is commanded (-1, 0) and keeps its rate-limit anchor; it still solves, as on the device.
    -> dict of per-step arrays: state [steps+1,8], cmd [steps,2], est (held), z, seen [steps,4], flags, blind, latch, status [steps]"""
    from oracle import waypoints as W, vehicle_sim as V
    import scenario as S
    p = O.params(8, weights if weights is not None else S.WEIGHTS)
    s = V.initial_state(1, X0, Y0, Psi0)
    s[0, 3] = VT
    sensor = np.zeros((1, 8)) if sensor_row is None else np.asarray(sensor_row, dtype=np.float64).reshape(1, 8)
    faults = np.asarray(fault_row, dtype=np.float64).reshape(1, WORDS)
    par = np.array([EST_Q + tuple(np.maximum(sensor[0, 0:4], EST_R))])
    plant = R.DEFAULT_ROW[None, :]
    rec, frec = np.zeros((1, 16)), np.zeros((1, WORDS))
    u_prev, U_prev, have_warm, latch = np.zeros(2), None, False, False
    states = np.zeros((steps + 1, 8))
    states[0] = s[0]
    log = dict(cmd=[], est=[], z=[], seen=[], flags=[], blind=[], latch=[], status=[])
    for k in range(steps):
        o = sense_faults(s, sensor, faults, frec, seed, k, gid)
        frec = o["rec"]
        seen = o["held"]
        if estimator:
            rec, seen, _, _ = E.estimate(rec, o["z"], s[:, 6:8], par, dt=0.1, gate=gate)
        x, y, psi, v = seen[0]
        xr, yr, pr, stop, _ci = W.get_waypoints(traj, x, y, psi, VT, traj_horizon=8)
        latch = bool(latch or stop or (blind_stop and o["blind"][0]))
        q = O.problem(p, [x, y, psi, v], np.stack([xr, yr, pr], 1), VT, u_prev)
        r = O.solve_condensed(p, q, o=O.opts(warm=1) if have_warm else O.opts(), U0=U_prev)
        U_prev, have_warm = r["U"].copy(), True
        if latch:
            cmd = np.array([-1.0, 0.0])
        else:
            cmd = r["U"][0].copy()
            u_prev = cmd.copy()
        for n, v_ in (("cmd", cmd), ("est", o["held"][0].copy()), ("z", o["z"][0].copy()), ("seen", seen[0].copy()), ("flags", o["flags"][0]),
                      ("blind", o["blind"][0]), ("latch", latch), ("status", r["status"])):
            log[n].append(v_)
        s, _ = R.update_plant(s, cmd[None, :], plant, n_updates=N_UPD)
        states[k + 1] = s[0]
    out = {n: np.array(v) for n, v in log.items()}
    out["state"] = states
    out["fault_record"] = frec[0]
    return out


def window_row(length, start=WINDOW[0], **words):
    """the neutral row with a GPS window; words: further KMPC_FAULT_* words by index"""
    row = NEUTRAL.copy()
    row[WIN_FROM], row[WIN_LEN] = start, length
    for k, v in words.items():
        row[int(k[1:])] = v
    return row


def max_ect(traj, state):
    """largest cross-track error of one vehicle's states [K,8] against the path's polyline [m]"""
    import scenario as S
    e, _ = S.cross_track(traj[:, 4:6], state[:, 0], state[:, 1])
    return float(np.abs(e).max())
