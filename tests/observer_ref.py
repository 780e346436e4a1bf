"""TEST INFRASTRUCTURE: numpy restatement of the disturbance observer and the command offset (kmpc_observe_batch, kmpc_cmd_offset_batch),
vectorised over the B vehicles and written from the text of include/kmpc.h, not from the kernel: kmpc_estimate_batch's filter on the solver's Euler
bicycle augmented with a course offset dpsi, a steering offset ddelta and an acceleration offset da; every new term appended after the estimator's.

observe(rec, z, u, params, ...) -> (rec, est, dist, innov, flags); model_step / jacobian / predict / update_channel are its parts, usable on their
own; cmd_offset(rec, latch, acc_cap, df_cap, cmd) -> cmd.  Also here: the inputs the CPU and the GPU tests share (single_call_case,
recursion_case) and the CPU closed loop (road_ref.cpu_loop's shape with the observer and the offset in it).
"""
import numpy as np

import estimator_ref as E
import road_ref as RR

NS, NP, WORDS, PAR_WORDS = 7, 28, 40, 16
COUNT, SKIPPED = 35, 36
SKIP, INIT, RESET = E.SKIP, E.INIT, E.RESET
L_A, L_B, PI = E.L_A, E.L_B, E.PI
wrap = E.wrap
TRI = {}                          # (i, j), i <= j -> index into the 28 words of P
for _i in range(NS):
    for _j in range(_i, NS):
        TRI[(_i, _j)] = len(TRI)
HAS = {0: (2, 3, 4, 5), 1: (2, 3, 4, 5), 2: (3, 5), 3: (6,)}     # the entries F has beside the identity, per row, in the order of the sums
BLOCK4 = [TRI[(i, j)] for i in range(4) for j in range(i, 4)]    # the ten words of the 4 x 4 block, in the estimator's order
# the defaults of vehicle_sim.DisturbanceObserver
Q, Q_DIST, R, P0 = (0.02, 0.02, 0.01, 0.1), (0.002, 0.002, 0.02), (0.2, 0.2, 0.02, 0.1), (0.05, 0.05, 0.5)
V_MIN, PSI_CAP, ACC_CAP, DF_CAP = 1.0, 0.2, 0.5, 0.1


def param_rows(B, q=Q, q_dist=Q_DIST, r=R, p0=P0):
    rows = np.zeros((B, PAR_WORDS))
    rows[:, 0:4], rows[:, 4:7], rows[:, 7:11], rows[:, 11:14] = q, q_dist, r, p0
    return rows


def pget(P, i, j):
    return P[:, TRI[(min(i, j), max(i, j))]]


def tri_to_full(P28):
    P28 = np.asarray(P28, dtype=np.float64)
    out = np.empty(P28.shape[:-1] + (NS, NS))
    for (i, j), k in TRI.items():
        out[..., i, j] = out[..., j, i] = P28[..., k]
    return out


def full_to_tri(P):
    return np.stack([P[..., i, j] for (i, j) in TRI], axis=-1)


def clip(a, cap):
    return RR.clip(a, cap)


def model_step(xh, u, dt, L_a=L_A, L_b=L_B):
    """one Euler step on xh [B,7] with u [B,2] -> (new xh, the header's intermediates); psi, v and the d's on the right are those before the step"""
    x, y, psi, v, dpsi, dde, da = (xh[:, i] for i in range(NS))
    de = u[:, 1] + dde
    t = np.tan(de)
    k = L_b / (L_a + L_b)
    beta = np.arctan(k * t)
    sb, cb = np.sin(beta), np.cos(beta)
    th = (psi + dpsi) + beta
    s, c = np.sin(th), np.cos(th)
    bp = k * (1.0 + t * t) / (1.0 + (k * t) * (k * t))
    vn = v + dt * (u[:, 0] + da)
    new = np.stack([x + dt * (v * c), y + dt * (v * s), wrap(psi + dt * (v / L_b * sb)), np.where(vn < 0.0, 0.0, vn), dpsi, dde, da], axis=1)
    return new, dict(s=s, c=c, sb=sb, cb=cb, bp=bp)


def f_entries(xh, u, dt, L_a=L_A, L_b=L_B):
    """{(i, k): [B]}: the entries F has beside the identity"""
    v = xh[:, 3]
    _, m = model_step(xh, u, dt, L_a, L_b)
    F = {(0, 2): -(dt * (v * m["s"])), (0, 3): dt * m["c"], (1, 2): dt * (v * m["c"]), (1, 3): dt * m["s"], (2, 3): dt * (m["sb"] / L_b)}
    F[(0, 4)], F[(1, 4)] = F[(0, 2)], F[(1, 2)]
    F[(0, 5)], F[(1, 5)] = F[(0, 2)] * m["bp"], F[(1, 2)] * m["bp"]
    F[(2, 5)] = dt * (v / L_b * (m["cb"] * m["bp"]))
    F[(3, 6)] = np.full(len(xh), dt)
    return F


def jacobian(xh, u, dt, L_a=L_A, L_b=L_B):
    """F [B,7,7]"""
    out = np.tile(np.eye(NS), (len(xh), 1, 1))
    for (i, k), f in f_entries(xh, u, dt, L_a, L_b).items():
        out[:, i, k] = f
    return out


def predict(xh, P28, u, q2, dt, v_min=0.0, L_a=L_A, L_b=L_B):
    """-> (xh, P28) after the step; q2 [B,7].  Only the upper triangle is formed, sums left to right as the header has them"""
    new, _ = model_step(xh, u, dt, L_a, L_b)
    F = f_entries(xh, u, dt, L_a, L_b)
    A = {}
    for i in range(4):
        for j in range(NS):
            a = pget(P28, i, j)
            for k in HAS[i]:
                a = a + F[(i, k)] * pget(P28, k, j)
            A[(i, j)] = a
    out = P28.copy()
    for i in range(4):
        for j in range(i, NS):
            p = A[(i, j)]
            if j < 4:
                for k in HAS[j]:
                    p = p + F[(j, k)] * A[(i, k)]
            out[:, TRI[(i, j)]] = p
    frozen = xh[:, 3] < v_min
    for i in range(NS):
        d = out[:, TRI[(i, i)]] + q2[:, i]
        out[:, TRI[(i, i)]] = np.where(frozen, out[:, TRI[(i, i)]], d) if i in (4, 5) else d
    return new, out


def update_channel(xh, P28, c, z_c, r2_c, gate=0.0):
    """one scalar update of channel c over seven states -> (xh, P28, innov [B], skipped [B] bool)"""
    with np.errstate(all="ignore"):
        nu = z_c - xh[:, c]
        if c == 2:
            nu = wrap(nu)
        S = P28[:, TRI[(c, c)]] + r2_c
        skip = ~np.isfinite(z_c) | ~((S > 0.0) & np.isfinite(S))
        if gate > 0.0:
            skip = skip | (nu * nu > gate * gate * S)
        col = np.stack([pget(P28, a, c) for a in range(NS)], axis=1)     # column c of P before this channel
        K = col / S[:, None]
        xn = xh + K * nu[:, None]
        Pn = P28.copy()
        for (a, b), k in TRI.items():
            Pn[:, k] = P28[:, k] - K[:, a] * col[:, b]
        innov = nu / np.sqrt(S)
    sk = skip[:, None]
    return np.where(sk, xh, xn), np.where(sk, P28, Pn), np.where(skip, 0.0, innov), skip


def observe(rec, z, u, params, dt=0.1, L_a=L_A, L_b=L_B, gate=0.0, v_min=V_MIN, psi_cap=PSI_CAP):
    """rec [B,40], z [B,4], u [B,2], params [B,16] -> (rec after the call, est [B,4], dist [B,3], innov [B,4], flags [B] int32)"""
    rec, z, u, params = (np.array(a, dtype=np.float64, copy=True) for a in (rec, z, u, params))
    B = len(rec)
    q2, r2, p02 = params[:, 0:7] * params[:, 0:7], params[:, 7:11] * params[:, 7:11], params[:, 11:14] * params[:, 11:14]
    first = rec[:, COUNT] == 0.0
    zfin = np.isfinite(z)
    with np.errstate(all="ignore"):
        xh, P = predict(rec[:, 0:7], rec[:, 7:35], u, q2, dt, v_min, L_a, L_b)
        innov, flags, nskip = np.zeros((B, 4)), np.zeros(B, dtype=np.int32), np.zeros(B)
        for c in range(4):
            xh, P, innov[:, c], sk = update_channel(xh, P, c, z[:, c], r2[:, c], gate)
            flags |= np.where(sk, SKIP[c], 0).astype(np.int32)
            nskip += sk
        xh[:, 2] = wrap(xh[:, 2])
        xh[:, 3] = np.where(xh[:, 3] < 0.0, 0.0, xh[:, 3])
        out = np.concatenate([xh, P, (rec[:, COUNT] + 1.0)[:, None], (rec[:, SKIPPED] + nskip)[:, None], np.zeros((B, 3))], axis=1)
    bad = ~np.isfinite(out).all(1)
    flags = np.where(bad, flags | RESET, flags).astype(np.int32)
    init = first & zfin.all(1)
    fresh_stays = first & ~zfin.all(1)
    first_rec = np.zeros((B, WORDS))
    first_rec[:, 0:4] = z
    for c in range(4):
        first_rec[:, 7 + TRI[(c, c)]] = r2[:, c]
    for a in range(3):
        first_rec[:, 7 + TRI[(4 + a, 4 + a)]] = p02[:, a]
    first_rec[:, COUNT] = 1.0
    out = np.where(init[:, None], first_rec, out)
    flags = np.where(init, INIT, flags)
    flags = np.where(fresh_stays, ((~zfin) * np.array(SKIP)).sum(1), flags).astype(np.int32)
    to_fresh = fresh_stays | (bad & ~first)
    out = np.where(to_fresh[:, None], 0.0, out)
    with np.errstate(all="ignore"):
        est = out[:, 0:4].copy()
        est[:, 2] = wrap(out[:, 2] + clip(out[:, 4], psi_cap))
    est = np.where((to_fresh | init)[:, None], z, est)
    innov = np.where((first | to_fresh)[:, None], 0.0, innov)
    return out, est, out[:, 4:7].copy(), innov, flags


def cmd_offset(rec, latch, acc_cap, df_cap, cmd):
    """-> cmd [B,2] after kmpc_cmd_offset_batch; latch [B] bool or None"""
    rec, cmd = np.asarray(rec, dtype=np.float64), np.array(cmd, dtype=np.float64, copy=True)
    dd, da = rec[:, 5], rec[:, 6]
    live = (rec[:, COUNT] != 0.0) & np.isfinite(dd) & np.isfinite(da)
    if latch is not None:
        live &= ~np.asarray(latch, dtype=bool)
    with np.errstate(invalid="ignore"):
        ca, cd = clip(da, acc_cap), clip(dd, df_cap)
        cmd[:, 0] = np.where(live & (ca != 0.0), cmd[:, 0] - ca, cmd[:, 0])
        cmd[:, 1] = np.where(live & (cd != 0.0), cmd[:, 1] - cd, cmd[:, 1])
    return cmd


def from_estimator(rec16):
    """an estimator record [B,16] as an observer record [B,40] with zero disturbances and zero covariance beyond the 4 x 4 block"""
    rec16 = np.asarray(rec16, dtype=np.float64)
    out = np.zeros((len(rec16), WORDS))
    out[:, 0:4] = rec16[:, 0:4]
    out[:, 7 + np.array(BLOCK4)] = rec16[:, 4:14]
    out[:, COUNT], out[:, SKIPPED] = rec16[:, 14], rec16[:, 15]
    return out


def reduced_params(par8):
    """estimator rows [B,8] -> observer rows [B,16] with q_dist = p0 = 0"""
    par8 = np.asarray(par8, dtype=np.float64)
    out = np.zeros((len(par8), PAR_WORDS))
    out[:, 0:4], out[:, 7:11] = par8[:, 0:4], par8[:, 4:8]
    return out


def to_estimator(rec40):
    """the estimator's 16 words of an observer record"""
    rec40 = np.asarray(rec40, dtype=np.float64)
    return np.concatenate([rec40[..., 0:4], rec40[..., 7 + np.array(BLOCK4)], rec40[..., COUNT:SKIPPED + 1]], axis=-1)


# ---------------------------------------------------------------- inputs shared by tests/test_observer_ref.py (CPU) and tests/test_observer.py (GPU)
def random_spd(rng, B, scale=(0.3, 0.3, 0.03, 0.2, 0.03, 0.02, 0.3)):
    """[B,7,7] covariances with standard deviations around `scale` and full correlations"""
    A = rng.normal(0, 1, (B, NS, NS))
    P = A @ A.transpose(0, 2, 1) / NS + 0.05 * np.eye(NS)
    d = np.asarray(scale) * rng.uniform(0.5, 2.0, (B, NS))
    return P * d[:, :, None] * d[:, None, :]


SINGLE_SEED, SINGLE_B, SINGLE_GATE = 53, 300, 3.0


def single_call_case():
    """B = 300 records in mid-run (two 256-thread blocks, the second a partial wave) with SPD P, disturbances of both signs, and the groups:
    [0, 20) psi-hat and z_psi on opposite sides of +-pi; [20, 40) one NaN channel (five vehicles per channel); [40, 60) an 8 sigma outlier in one
    channel under gate = 3; [60, 70) fresh records, of which 68 and 69 get a non-finite measurement; [70, 100) slow vehicles, v < v_min (a third
    of them standing).  The measurement is pred + L n with L the Cholesky factor of the 4 x 4 block of P_pred + R, as estimator_ref's case.
    -> dict(rec, z, u, params, gate, dt, v_min, psi_cap)"""
    rng = np.random.default_rng(SINGLE_SEED)
    B = SINGLE_B
    rec = np.zeros((B, WORDS))
    rec[:, 0:2] = rng.uniform(-500, 500, (B, 2))
    rec[:, 2] = rng.uniform(-np.pi, np.pi, B)
    rec[:, 3] = rng.uniform(2, 20, B)
    rec[70:100, 3] = np.where(np.arange(30) % 3 == 0, 0.0, rng.uniform(0.0, 0.99, 30))
    rec[:, 4:7] = rng.uniform(-1, 1, (B, 3)) * np.array([0.3, 0.05, 0.8])      # dpsi beyond psi_cap = 0.2 in a third of the vehicles
    rec[:, 7:35] = full_to_tri(random_spd(rng, B))
    rec[:, COUNT] = rng.integers(1, 500, B)
    rec[:, SKIPPED] = rng.integers(0, 7, B)
    params = np.zeros((B, PAR_WORDS))
    params[:, 0:14] = np.array(Q + Q_DIST + R + P0) * rng.uniform(0.5, 2.0, (B, 14))
    u = np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.5, 0.5, B)], 1)
    u[0:20, 1] = 0.0
    rec[0:20, 5] = 0.0                                                          # no steering at all: the predict leaves psi-hat where it is
    rec[0:20, 2] = np.where(np.arange(20) % 2 == 0, 1.0, -1.0) * (PI - 1e-6)
    n = np.clip(rng.normal(0, 1, (B, 4)), -2.0, 2.0)
    for k in range(20):
        n[40 + k, k % 4] = 8.0 if k % 8 < 4 else -8.0
    pred, Ppred = predict(rec[:, 0:7], rec[:, 7:35], u, params[:, 0:7] ** 2, 0.1, V_MIN)
    S = tri_to_full(Ppred)[:, 0:4, 0:4].copy()
    S[:, range(4), range(4)] += params[:, 7:11] ** 2
    delta = np.einsum("bij,bj->bi", np.linalg.cholesky(S), n)
    flip = np.sign(delta[0:20, 2]) != np.sign(rec[0:20, 2])
    delta[0:20][flip] *= -1.0
    z = pred[:, 0:4] + delta
    z[:, 2] = wrap(z[:, 2])
    z[:, 3] = np.maximum(z[:, 3], 0.0)
    for k in range(20):
        z[20 + k, k % 4] = np.nan
    rec[60:70] = 0.0
    z[68, 1] = np.nan
    z[69, 3] = np.inf
    return dict(rec=rec, z=z, u=u, params=params, gate=SINGLE_GATE, dt=0.1, v_min=V_MIN, psi_cap=PSI_CAP)


RUN_SEED, RUN_B, RUN_STEPS = 59, 65, 100


def recursion_case():
    """65 vehicles (one wave and one lane) x 100 periods, open loop: the truth from the augmented model with constant disturbances per vehicle (both
    signs), process noise N(0, q^2) on the four states, measurements with sigma = R; vehicles 60 ... 64 drive below v_min.
    -> dict(z [K,B,4], u [B,2], params [B,16], d [B,3])"""
    rng = np.random.default_rng(RUN_SEED)
    B, K = RUN_B, RUN_STEPS
    q, r = np.array(Q), np.array(R)
    d = rng.uniform(-1, 1, (B, 3)) * np.array([0.05, 0.03, 0.5])
    x = np.concatenate([np.stack([rng.uniform(-500, 500, B), rng.uniform(-500, 500, B), rng.uniform(-np.pi, np.pi, B), rng.uniform(4, 12, B)], 1), d], 1)
    x[60:, 3] = rng.uniform(0.2, 0.8, 5)
    u = np.stack([-d[:, 2] + rng.uniform(-0.02, 0.02, B), rng.uniform(-0.1, 0.1, B)], 1)     # acc + da stays small: the speeds stay where they start
    z = np.empty((K, B, 4))
    for k in range(K):
        if k:
            x, _ = model_step(x, u, 0.1)
            x[:, 0:4] = x[:, 0:4] + q * rng.normal(0, 1, (B, 4))
            x[:, 2] = wrap(x[:, 2])
            x[:, 3] = np.maximum(x[:, 3], 0.0)
        z[k] = x[:, 0:4] + r * rng.normal(0, 1, (B, 4))
        z[k, :, 2] = wrap(z[k, :, 2])
        z[k, :, 3] = np.maximum(z[k, :, 3], 0.0)
    return dict(z=z, u=u, params=param_rows(B), d=d)


def run_recursion(z, u, params, gate=0.0, dt=0.1, v_min=V_MIN, psi_cap=PSI_CAP):
    """the restatement over z [K,B,4] from fresh records -> dict(rec [K,B,40], est [K,B,4], dist [K,B,3], innov [K,B,4], flags [K,B])"""
    K1, B = z.shape[0], z.shape[1]
    rec = np.zeros((B, WORDS))
    out = dict(rec=np.empty((K1, B, WORDS)), est=np.empty((K1, B, 4)), dist=np.empty((K1, B, 3)), innov=np.empty((K1, B, 4)),
               flags=np.empty((K1, B), dtype=np.int32))
    for k in range(K1):
        rec, out["est"][k], out["dist"][k], out["innov"][k], out["flags"][k] = observe(rec, z[k], u, params, dt=dt, gate=gate, v_min=v_min, psi_cap=psi_cap)
        out["rec"][k] = rec
    return out


# ---------------------------------------------------------------- the closed loop of the issue's table
LOOP_ROADS = (dict(), dict(a_lat=1.5), dict(df_offset=0.03), dict(a_long=-0.5), dict(a_lat=1.5, df_offset=0.03))
LOOP_NAMES = ("neutral", "a_lat=1.5", "df_offset=0.03", "a_long=-0.5", "a_lat=1.5, df_offset=0.03")
LATERAL = (1, 2, 4)               # the laterally disturbed rows
LOOP_STEPS, TAIL = 200, 100


def cpu_loop(O, traj, X0, Y0, Psi0, road_row, steps=LOOP_STEPS, mode="observer", obs=None):
    """road_ref.cpu_loop with a stage between the truth and the controller: mode "none" (road_ref.cpu_loop itself), "estimator" (estimator_ref.estimate
    with Estimator's defaults) or "observer" (observe + cmd_offset with DisturbanceObserver's defaults, or the keywords in `obs`: q, q_dist, r, p0,
    v_min, psi_cap, acc_cap, df_cap).  The filters read the truth as their measurement and the plant's actuator states as their input; the solver's
    rate-limit anchor stays the solver's own command; the plant gets the command after the offset.
    -> road_ref.cpu_loop's dict, plus dist [steps,3] (observer) and seen [steps,4]"""
    from oracle import waypoints as W, vehicle_sim as Vs
    import plant_ref as R_
    import scenario as S
    o = dict(q=Q, q_dist=Q_DIST, r=R, p0=P0, v_min=V_MIN, psi_cap=PSI_CAP, acc_cap=ACC_CAP, df_cap=DF_CAP)
    o.update(obs or {})
    p = O.params(8, S.WEIGHTS)
    s = Vs.initial_state(1, X0, Y0, Psi0)
    s[0, 3] = RR.VT
    plant, road = R_.DEFAULT_ROW[None, :], np.asarray(road_row, dtype=np.float64)[None, :]
    u_prev, U_prev, have_warm = np.zeros(2), None, False
    cmds, states, status = np.zeros((steps, 1, 2)), np.zeros((steps + 1, 1, 8)), []
    states[0] = s
    stat, near = np.zeros((1, 4)), np.zeros(1, dtype=bool)
    rec40, rec16 = np.zeros((1, WORDS)), np.zeros((1, 16))
    par16, par8 = param_rows(1, o["q"], o["q_dist"], o["r"], o["p0"]), np.array([tuple(o["q"]) + tuple(o["r"])])
    dist, seen_log = np.zeros((steps, 3)), np.zeros((steps, 4))
    for k in range(steps):
        z = s[:, 0:4].copy()
        if mode == "observer":
            rec40, seen, dist[k:k + 1], _, _ = observe(rec40, z, s[:, 6:8], par16, dt=0.1, v_min=o["v_min"], psi_cap=o["psi_cap"])
        elif mode == "estimator":
            rec16, seen, _, _ = E.estimate(rec16, z, s[:, 6:8], par8, dt=0.1)
        else:
            seen = z
        seen_log[k] = seen[0]
        x, y, psi, v = seen[0]
        xr, yr, pr, _stop, _ci = W.get_waypoints(traj, x, y, psi, RR.VT, traj_horizon=8)
        q = O.problem(p, [x, y, psi, v], np.stack([xr, yr, pr], 1), RR.VT, u_prev)
        r = O.solve_condensed(p, q, o=O.opts(warm=1) if have_warm else O.opts(), U0=U_prev)
        cmd = r["U"][0].copy()
        u_prev, U_prev, have_warm = cmd.copy(), r["U"].copy(), True
        if mode == "observer":
            cmd = cmd_offset(rec40, None, o["acc_cap"], o["df_cap"], cmd[None, :])[0]
        cmds[k, 0] = cmd
        status.append(r["status"])
        s, stat = RR.advance_road(s, cmds, k, plant, road, [0], 2, RR.N_UPD, stat=stat, near=near)
        states[k + 1] = s
    ect, _ = S.cross_track(traj[:, 4:6], states[:, 0, 0], states[:, 0, 1])
    return dict(state=states[:, 0], cmd=cmds[:, 0], status=np.array(status), stat=stat[0], near=bool(near[0]), ect=ect, dist=dist, seen=seen_log)


_LOOPS = {}


def cpu_loops(O, roads, offsets=(0.0,), steps=LOOP_STEPS, modes=("none", "observer")):
    """road indices (into LOOP_ROADS) x lateral offsets x modes, computed once per process -> {(road index, offset, mode): cpu_loop's dict}, trajectory"""
    X0, Y0, P0_, tr = RR.loop_start(offsets)
    out = {}
    for ri in roads:
        for oi, off in enumerate(offsets):
            for mode in modes:
                key = (ri, off, mode, steps)
                if key not in _LOOPS:
                    _LOOPS[key] = cpu_loop(O, tr, X0[oi], Y0[oi], P0_[oi], RR.rows(1, **LOOP_ROADS[ri])[0], steps=steps, mode=mode)
                out[(ri, off, mode)] = _LOOPS[key]
    return out, tr
