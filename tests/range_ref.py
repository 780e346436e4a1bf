"""TEST INFRASTRUCTURE: numpy restatement of the range sensor and leader tracker (kmpc_range_follow_batch), written from the text of
include/kmpc_range.h, not from the kernel: the draws with plant_ref's Philox, detection, measurement, the track's predict and two scalar updates
operation by operation, follow_ref's law on what the track believes, the record; the seeded draw that tests/test_range_ref.py and
tests/test_range.py share; and follow_ref's CPU platoon with the stage behind the search.
"""
import numpy as np

import follow_ref as FR
import plant_ref as R

FIELDS = ("range_max", "sigma_r", "sigma_v", "bias_r", "p_drop", "filter", "coast_max", "q_gap", "q_v", "r_gap", "r_v")
REC_FIELDS = ("gap_hat", "v_hat", "p00", "p01", "p11", "track_id", "coast", "n", "n_detect", "n_drop", "n_out", "n_new", "n_lost", "n_bound",
              "sum_egap2", "max_egap")
WORDS = 16
DEFAULT_ROW = np.array([120.0, 0.25, 0.12, 0.0, 0.0, 1.0, 5.0, 0.01, 0.25, 0.0625, 0.0144, 0.0, 0.0, 0.0, 0.0, 0.0])
NEUTRAL = dict(range_max=np.inf, sigma_r=0.0, sigma_v=0.0, bias_r=0.0, p_drop=0.0, filter=0.0, coast_max=0.0)
TAG = 0x20000000
(GAP_HAT, V_HAT, P00, P01, P11, TRACK_ID, COAST, N, N_DETECT, N_DROP, N_OUT, N_NEW, N_LOST, N_BOUND, SUM_EGAP2, MAX_EGAP) = range(16)


def rows(B, **kw):
    """[B,16] sensor rows: the default, with any of FIELDS a scalar or one value per vehicle"""
    r = np.tile(DEFAULT_ROW, (B, 1))
    for k, v in kw.items():
        r[:, FIELDS.index(k)] = v
    return r


def neutral_rows(B):
    return rows(B, **NEUTRAL)


def fresh_rec(B):
    rec = np.zeros((B, WORDS))
    rec[:, TRACK_ID] = -1.0
    return rec


def draws(B, seed, period, id_base=0):
    """-> n0 [B], n1 [B], u [B]: the header's step 1"""
    gid = (np.arange(B, dtype=np.uint64) + np.uint64(id_base & 0xFFFFFFFFFFFFFFFF))
    m = np.uint64(R.M32)
    ctr = (gid & m, gid >> np.uint64(32), np.full(B, period & R.M32, dtype=np.uint64), np.full(B, ((period >> 32) & R.M32) ^ TAG, dtype=np.uint64))
    w = R.philox4x32_10(ctr, (np.uint64(seed & R.M32), np.uint64((seed >> 32) & R.M32)))
    u0, u1, u2 = ((np.asarray(x, dtype=np.uint64).astype(np.float64) + 0.5) * 2.0 ** -32 for x in w[:3])
    r, a = np.sqrt(-2.0 * np.log(u0)), 6.283185307179586 * u1
    return r * np.cos(a), r * np.sin(a), u2


def step(truth, leader, v_true, v_known, follow_rows, range_rows, seed, period, id_base, v_cap, rec, dt):
    """one call of kmpc_range_follow_batch -> dict v_out [B], rec [B,16] (a new array), meas [B,4], det, drop, out, new, lost, track, bound [B]
    bool, margin [B] (|v_f - cap| with a track, +inf without: how far the law's speed is from switching N_BOUND), safe_arm [B] (the output is the
    sqrt arm's value)"""
    truth, v_t, v_k, cap = (np.asarray(a, dtype=np.float64) for a in (truth, v_true, v_known, v_cap))
    fr, rr, r = (np.asarray(a, dtype=np.float64) for a in (follow_rows, range_rows, rec))
    L = np.asarray(leader).astype(np.int64)
    B = len(L)
    gap, v_j = truth[:, 0], truth[:, 1]
    rmax, sig_r, sig_v, bias, p_drop, filt, coast_max, q_gap, q_v, r_gap, r_v = (rr[:, i] for i in range(11))
    n0, n1, u = draws(B, seed, period, id_base)
    with np.errstate(all="ignore"):
        known_ok = np.isfinite(v_k)
        valid = (L >= 0) & np.isfinite(gap) & np.isfinite(v_j) & np.isfinite(v_t) & known_ok
        inr = valid & (gap <= rmax)
        drop = inr & (u < p_drop)
        det = inr & ~drop
        z_r = gap.copy()
        z_r = np.where(bias != 0.0, z_r + bias, z_r)
        z_r = np.where(sig_r != 0.0, z_r + sig_r * n0, z_r)
        e = v_k - v_t
        z_v = np.where(e != 0.0, v_j + e, v_j)
        z_v = np.where(sig_v != 0.0, z_v + sig_v * n1, z_v)

        g, v, p00, p01, p11, tid, coast = (r[:, i].copy() for i in range(7))
        Ld = L.astype(np.float64)
        new = det & (tid != Ld)
        old = ~new & (tid >= 0.0)
        # predict
        gp_ = g + dt * (v - v_k)
        t = dt * p11
        a00 = (p00 + dt * (2.0 * p01 + t)) + q_gap
        a01 = p01 + t
        a11 = p11 + q_v
        g, p00, p01, p11 = (np.where(old, x, y) for x, y in ((gp_, g), (a00, p00), (a01, p01), (a11, p11)))
        upd = old & det
        raw, kal = upd & (filt == 0.0), upd & (filt != 0.0)
        # the range update
        S = p00 + r_gap
        k0, k1, y = p00 / S, p01 / S, z_r - g
        gains = [k0, k1]
        g1, v1 = g + k0 * y, v + k1 * y
        b11, b01, b00 = p11 - k1 * p01, p01 - k0 * p01, p00 - k0 * p00
        # the speed update
        S = b11 + r_v
        k0, k1, y = b01 / S, b11 / S, z_v - v1
        gains += [k0, k1]
        g2, v2 = g1 + k0 * y, v1 + k1 * y
        c00, c01, c11 = b00 - k0 * b01, b01 - k1 * b01, b11 - k1 * b11
        g, v = np.where(kal, g2, g), np.where(kal, v2, v)
        p00, p01, p11 = np.where(kal, c00, p00), np.where(kal, c01, p01), np.where(kal, c11, p11)
        g, v = np.where(raw | new, z_r, g), np.where(raw | new, z_v, v)
        p00, p01, p11 = np.where(new, r_gap, p00), np.where(new, 0.0, p01), np.where(new, r_v, p11)
        miss = old & ~det
        coast = np.where(new | upd, 0.0, np.where(miss, coast + 1.0, coast))
        lost = miss & ((coast > coast_max) | (tid != Ld) | ~known_ok)
        tid = np.where(new, Ld, np.where(lost, -1.0, tid))

        track = tid >= 0.0
        o = _law(g, v_k, v, fr, cap)
        bound = track & o["bound"]
        v_out = np.where(bound, o["v_f"], cap)
        safe_arm = bound & ~(o["v_gap"] < o["v_safe"]) & (o["v_safe"] > 0.0)
        margin = np.where(track, np.abs(o["v_f"] - cap), np.inf)
        err = g - gap
        e_ok = track & np.isfinite(err)
        out = r.copy()
        out[:, GAP_HAT], out[:, V_HAT], out[:, P00], out[:, P01], out[:, P11], out[:, TRACK_ID], out[:, COAST] = g, v, p00, p01, p11, tid, coast
        out[:, N] += 1.0
        out[:, N_DETECT] += det
        out[:, N_DROP] += drop
        out[:, N_OUT] += valid & ~inr
        out[:, N_NEW] += new
        out[:, N_LOST] += lost
        out[:, N_BOUND] += bound
        out[:, SUM_EGAP2] = np.where(e_ok, out[:, SUM_EGAP2] + err * err, out[:, SUM_EGAP2])
        out[:, MAX_EGAP] = np.where(e_ok & (np.abs(err) > out[:, MAX_EGAP]), np.abs(err), out[:, MAX_EGAP])
    meas = np.stack([np.where(det, z_r, np.nan), np.where(det, z_v, np.nan), det.astype(np.float64), coast], 1)
    return dict(v_out=v_out, rec=out, meas=meas, det=det, drop=drop, out=valid & ~inr, new=new, lost=lost, track=track, bound=bound, margin=margin,
                safe_arm=safe_arm, rad=o["rad"], at=o["at"], v_f=o["v_f"], old=old, raw=raw, kal=kal, gains=gains, z_r=z_r, z_v=z_v, truth_gap=gap)


def _law(gap, v_b, v_j, row, v_cap):
    """follow_ref.law on a GIVEN gap: its first operation, gap = diff - LENGTH, is skipped by handing it a row whose LENGTH is 0 (x - 0 == x, bit
    for bit, -0 aside, which no comparison below tells from +0)"""
    row0 = np.array(row, dtype=np.float64)
    row0[:, 4] = 0.0
    return FR.law(gap, v_b, v_j, row0, v_cap)


# ---------------------------------------------------------------- the seeded draws shared by the CPU and the GPU tests
SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)     # block and wave edges of a 256-thread elementwise kernel
DT = 0.1


def draw(B, seed=0, noisy=True, calls=3):
    """B vehicles over `calls` consecutive calls: true gaps U(-2, 150) m that move by the speeds' difference from call to call, speeds U(0, 12) m/s,
    v_cap U(2, 12), follow_ref's random follow rows, random sensor rows (RANGE_MAX U(20, 140) or +inf, BIAS_R 0 or U(-0.5, 0.5), P_DROP 0 or 0.3,
    FILTER 0 / 1, COAST_MAX 0 ... 3, Q and R log-uniform, words 11 ... 15 junk; with noisy the sigmas U(0, 1) or 0, else 0); 5 % of the vehicles
    have no leader, 5 % non-finite truth or speeds in some call, and the leader index changes between calls for 10 %.
    -> dict follow_rows [B,8], range_rows [B,16], v_cap [B], and per call lists truth [B,2], leader [B] int32, v_true [B], v_known [B]"""
    rng = np.random.default_rng(7000 * B + seed)
    fr = FR.draw(B, seed, paths=0, bad=False)["rows"]
    rr = np.tile(DEFAULT_ROW, (B, 1))
    rr[:, 0] = np.where(rng.random(B) < 0.3, np.inf, rng.uniform(20.0, 140.0, B))
    rr[:, 1] = np.where(rng.random(B) < 0.8, rng.uniform(0.0, 1.0, B), 0.0) if noisy else 0.0
    rr[:, 2] = np.where(rng.random(B) < 0.8, rng.uniform(0.0, 1.0, B), 0.0) if noisy else 0.0
    rr[:, 3] = np.where(rng.random(B) < 0.5, rng.uniform(-0.5, 0.5, B), 0.0)
    rr[:, 4] = np.where(rng.random(B) < 0.5, 0.3, 0.0)
    rr[:, 5] = rng.integers(0, 2, B)
    rr[:, 6] = rng.integers(0, 4, B)
    rr[:, 7:11] = 10.0 ** rng.uniform(-3.0, 0.0, (B, 4))
    rr[:, 11:16] = rng.uniform(-9, 9, (B, 5))
    v_cap = rng.uniform(2.0, 12.0, B)
    gap, v_j, v_b = rng.uniform(-2.0, 150.0, B), rng.uniform(0.0, 12.0, B), rng.uniform(0.0, 12.0, B)
    lead = rng.integers(0, max(B, 2), B).astype(np.int32)
    none = rng.random(B) < 0.05
    changes = rng.random(B) < 0.10
    junk = np.array([np.nan, np.inf, -np.inf])
    truth, leader, v_true, v_known = [], [], [], []
    for c in range(calls):
        if c:
            gap = gap + DT * (v_j - v_b)
            lead = np.where(changes, (lead + 1 + c).astype(np.int32), lead).astype(np.int32)
        t = np.stack([gap, v_j], 1)
        vt = v_b.copy()
        vk = np.where(rng.random(B) < 0.5, vt, vt + rng.uniform(-0.2, 0.2, B))
        hit = rng.random(B) < 0.05
        which = rng.integers(0, 4, B)
        bad = junk[rng.integers(0, 3, B)]
        t[hit & (which == 0), 0] = bad[hit & (which == 0)]
        t[hit & (which == 1), 1] = bad[hit & (which == 1)]
        vt[hit & (which == 2)] = bad[hit & (which == 2)]
        vk[hit & (which == 3)] = bad[hit & (which == 3)]
        ld = np.where(none, -1, lead).astype(np.int32)
        t[ld < 0] = (np.inf, 0.0)          # what kmpc_follow_fleet writes without a leader
        truth.append(t); leader.append(ld); v_true.append(vt); v_known.append(vk)
    return dict(follow_rows=fr, range_rows=rr, v_cap=v_cap, truth=truth, leader=leader, v_true=v_true, v_known=v_known)


def run(d, seed=5, period0=11, id_base=0, rec=None, sl=slice(None)):
    """the calls of a draw in sequence on one record -> list of step() dicts (vehicles `sl` of the draw, drawn as vehicles id_base + ...)"""
    rec = fresh_rec(len(d["v_cap"][sl])) if rec is None else rec
    outs = []
    for c in range(len(d["truth"])):
        o = step(d["truth"][c][sl], d["leader"][c][sl], d["v_true"][c][sl], d["v_known"][c][sl], d["follow_rows"][sl], d["range_rows"][sl], seed,
                 period0 + c, id_base, d["v_cap"][sl], rec, DT)
        rec = o["rec"]
        outs.append(o)
    return outs


# ---------------------------------------------------------------- how far a device run may lie from the restatement
TOL_N = 1e-13     # one normal of the device against numpy's (tests/test_plant_sensor.py: log / sqrt / cos / sin within a few ulp each, |n| < 6.8)
ROUND = 8.0       # correctly rounded operations on inputs that differ: each may round the other way, one ulp of its result; the chain from the
                  # record to any output word of one call is at most eight operations long


def _f(a):
    return np.nan_to_num(np.abs(a), nan=0.0, posinf=0.0, neginf=0.0)


def bounds(follow_rows, range_rows, outs, dt):
    """the derived bound of tests/test_range.py's noisy parity, per call of `outs` (step()'s dicts of consecutive calls from a fresh record, or from
    one that is exact) -> list of dicts z_r, z_v, gap_hat, v_hat, v_out, sum_egap2, max_egap [B].  P, the gains, the counters and the track are
    functions of the rows, the truth and integer draws: no allowance.  Per call, with dr = TOL_N * SIGMA_R + ulp(z_r) and dv likewise:
      a new track or FILTER = 0:  e_g = dr, e_v = dv                     (the state IS the measurement)
      predict:                     e_g += dt * e_v                        (dt couples the speed error into the gap)
      range update:                e_v += |k1| (dr + e_g);  e_g = |1 - k0| e_g + |k0| dr       (the restatement's own gains: they are exact)
      speed update:                e_g += |k0| (dv + e_v);  e_v = |1 - k1| e_v + |k1| dv
    plus ROUND ulp of the largest magnitude in the chain.  The law is 1-Lipschitz in its two arms (min, max and the cap do not amplify):
      v_gap:  e_v + K_GAP e_g;   v_safe:  d = 2 |V_HAT| e_v + e_v^2 + 2 A_BRAKE e_g under the root, |sqrt(x + d) - sqrt(x)| <= min(d / sqrt(x),
      sqrt(d)), plus tests/test_follow.py's 2 ulp of the square-root term.  The error words: e = GAP_HAT - gap moves by e_g, its square by
      2 |e| e_g + e_g^2, summed over the calls; the largest by the largest e_g."""
    fr, rr = np.asarray(follow_rows, dtype=np.float64), np.asarray(range_rows, dtype=np.float64)
    B = len(fr)
    e_g, e_v, e_sum, e_max = np.zeros(B), np.zeros(B), np.zeros(B), np.zeros(B)
    res = []
    with np.errstate(all="ignore"):
        for o in outs:
            rec = o["rec"]
            g, v = rec[:, GAP_HAT], rec[:, V_HAT]
            dr = np.where(o["det"], TOL_N * rr[:, 1] + np.spacing(_f(o["z_r"])), 0.0)
            dv = np.where(o["det"], TOL_N * rr[:, 2] + np.spacing(_f(o["z_v"])), 0.0)
            k0r, k1r, k0v, k1v = (_f(k) for k in o["gains"])
            a0r, a1v = _f(1.0 - o["gains"][0]), _f(1.0 - o["gains"][3])
            pg = e_g + dt * e_v
            v1 = e_v + k1r * (dr + pg)
            g1 = a0r * pg + k0r * dr
            g2 = g1 + k0v * (dv + v1)
            v2 = a1v * v1 + k1v * dv
            state = o["new"] | o["raw"]
            slack = ROUND * np.spacing(np.maximum(np.maximum(_f(g), _f(o["z_r"])), np.maximum(_f(v), 1.0)))
            e_g = np.where(state, dr, np.where(o["kal"], g2 + slack, np.where(o["old"], pg + slack, e_g)))
            e_v = np.where(state, dv, np.where(o["kal"], v2 + slack, e_v))
            d_gap = e_v + fr[:, 3] * e_g
            d = 2.0 * _f(v) * e_v + e_v * e_v + 2.0 * fr[:, 2] * e_g
            root = np.sqrt(_f(o["rad"]))
            d_safe = np.minimum(np.where(root > 0.0, d / root, np.inf), np.sqrt(d)) + 2.0 * np.spacing(root)
            law_slack = ROUND * np.spacing(np.maximum(np.maximum(_f(g), _f(v)), np.maximum(root, 1.0)))
            e_out = np.where(o["track"], np.maximum(d_gap, d_safe) + law_slack, 0.0)
            err = _f(g - o["truth_gap"])
            d_err = e_g + np.spacing(err)
            ok = o["track"] & np.isfinite(g - o["truth_gap"])
            e_sum = e_sum + np.where(ok, 2.0 * err * d_err + d_err * d_err + np.spacing(_f(rec[:, SUM_EGAP2])), 0.0)
            e_max = np.where(ok, np.maximum(e_max, d_err), e_max)
            res.append(dict(z_r=dr, z_v=dv, gap_hat=e_g, v_hat=e_v, v_out=e_out, sum_egap2=e_sum.copy(), max_egap=e_max.copy()))
    return res


# ---------------------------------------------------------------- the CPU platoon loop with the stage behind the search
def cpu_platoon(O, traj, start, targets, follow_rows, range_rows, seed=0, steps=150, known=None):
    """follow_ref.cpu_platoon with kmpc_range_follow_batch's restatement behind follow(): the same pieces in the same order, v_follow = the
    stage's cap.  known(k, state) -> [B] the followers' speeds as their controllers know them (None: the truth's).
    -> cpu_platoon's dict plus rec [B,16], meas [steps,B,4], gap_seen, v_lead_seen [steps,B], v_ideal [steps,B]"""
    from oracle import waypoints as W, vehicle_sim as Vs
    import road_ref as RR
    import scenario as S
    import track_score_ref as TS
    B = len(start)
    targets = np.asarray(targets, dtype=np.float64)
    p = O.params(8, S.WEIGHTS)
    s = np.concatenate([Vs.initial_state(1, traj[i, 4], traj[i, 5], traj[i, 3]) for i in start])
    s[:, 3] = targets
    plant, road = np.tile(R.DEFAULT_ROW, (B, 1)), np.tile(RR.NEUTRAL_ROW, (B, 1))
    frows = np.asarray(follow_rows, dtype=np.float64)
    u_prev, U_prev, have_warm = np.zeros((B, 2)), [None] * B, False
    cmds, states = np.zeros((steps, B, 2)), np.zeros((steps + 1, B, 8))
    status, leader = np.zeros((steps, B), dtype=np.int64), np.zeros((steps, B), dtype=np.int64)
    v_follow, gap, v_ideal, gap_seen, v_lead_seen = (np.zeros((steps, B)) for _ in range(5))
    meas = np.zeros((steps, B, 4))
    states[0] = s
    pstat, near, fstat, rec, stop_any = np.zeros((B, 4)), np.zeros(B, dtype=bool), FR.fresh_stat(B), fresh_rec(B), False

    def see(state, stat):
        s_along = TS.errors(traj, state[:, 0], state[:, 1], state[:, 2])["s_along"]
        return FR.follow(s_along, state[:, 3], None, None, frows, targets, stat)
    for k in range(steps):
        f = see(s, fstat)
        fstat = f["stat"]
        vk = s[:, 3] if known is None else known(k, s)
        o = step(np.stack([f["gap"], f["v_lead"]], 1), f["leader"], s[:, 3], vk, frows, range_rows, seed, k, 0, targets, rec, 0.01 * FR.N_UPD)
        rec = o["rec"]
        v_follow[k], gap[k], leader[k], v_ideal[k], meas[k] = o["v_out"], f["gap"], f["leader"], f["v_out"], o["meas"]
        gap_seen[k], v_lead_seen[k] = np.where(o["track"], rec[:, GAP_HAT], np.inf), np.where(o["track"], rec[:, V_HAT], 0.0)
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
        s, pstat = RR.advance_road(s, cmds, k, plant, road, [0] * B, 2, FR.N_UPD, stat=pstat, near=near)
        states[k + 1] = s
    return dict(state=states, cmd=cmds, status=status, v_follow=v_follow, gap=gap, leader=leader, stat=fstat, stop=stop_any,
                final_gap=see(s, None)["gap"], rec=rec, meas=meas, gap_seen=gap_seen, v_lead_seen=v_lead_seen, v_ideal=v_ideal)


_cache = {}


def cached_platoon(O, case, key, range_rows, steps=150):
    """a case of follow_ref.CASES with the stage, computed once per process and `key` -> (cpu_platoon's dict, trajectory, start indices)"""
    import fleet_scenario as F
    c = FR.CASES[case]
    tr = F.trajectory(c["path"])
    start = FR.platoon_start(tr, c["spacing"], len(c["targets"]))
    if (case, key, steps) not in _cache:
        _cache[(case, key, steps)] = cpu_platoon(O, tr, start, c["targets"], FR.rows(len(start), **c["row"]), range_rows, steps=steps)
    return _cache[(case, key, steps)], tr, start
