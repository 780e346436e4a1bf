"""TEST INFRASTRUCTURE: numpy restatement of the lane stage (kmpc_lane_step_fleet, kmpc_ref_offset_batch), written from the text of
include/kmpc_lanes.h, not from the kernel: the five searches as masked argmins per vehicle, follow_ref's law for the own leader and for the sides,
the squared Gipps safety tests, the decision with its parity rule, the ramp and the record; the seeded draw that tests/test_lanes_ref.py and
tests/test_lanes.py share (follow_ref.draw with lanes, vehicles in mid-change and e_ct near the lane centres); and a CPU overtaking loop on
follow_ref.cpu_platoon's parts (the oracle's waypoints and solver, the track score's restated arclength and cross-track error, road_ref's plant).
"""
import numpy as np

import follow_ref as FR
import plant_ref as R
import road_ref as RR
import track_score_ref as TS

FIELDS = ("n_lanes", "width", "v_lat", "gain", "hold", "clear_tol", "keep_right")
REC_FIELDS = ("lane", "lane_from", "offset", "hold_left", "n", "n_leader", "n_bound", "n_contact", "min_gap", "max_closing", "n_changes",
              "sum_elane2", "max_elane")
DEFAULT_ROW = np.array([1.0, 3.5, 1.0, 0.5, 20.0, 0.5, 1.0, 0.0])
LANE, LANE_FROM, OFFSET, HOLD_LEFT, N, N_LEADER, N_BOUND, N_CONTACT, MIN_GAP, MAX_CLOSING, N_CHANGES, SUM_ELANE2, MAX_ELANE = range(13)


def rows(B, **kw):
    """[B,8] lane rows: the default, with any of FIELDS a scalar or one value per vehicle"""
    r = np.tile(DEFAULT_ROW, (B, 1))
    for k, v in kw.items():
        r[:, FIELDS.index(k)] = v
    return r


def fresh_rec(B, lane0=None, width=3.5):
    rec = np.zeros((B, 16))
    rec[:, MIN_GAP] = np.inf
    if lane0 is not None:
        rec[:, LANE] = rec[:, LANE_FROM] = lane0
        rec[:, OFFSET] = np.asarray(lane0, dtype=np.float64) * width
    return rec


def bit(x):
    """bit(x) of a lane word: 1 << (int)x when 0 <= x <= 31, else 0; arrays or scalars -> uint32"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = (x >= 0.0) & (x <= 31.0)
    return np.where(ok, np.left_shift(np.uint64(1), np.where(ok, x, 0.0).astype(np.uint64)), np.uint64(0)).astype(np.uint32)


def _side_law(d, v_b, v_j, row, cap):
    """follow_ref.law for ONE pair -> dict of scalars"""
    o = FR.law(np.array([d]), np.array([v_b]), np.array([v_j]), row[None, :], np.array([cap]))
    return {k: v[0] for k, v in o.items()}


def step(s, e_ct, v, path_id, present, follow_rows, lane_rows, v_cap, occ_in, rec, k, dt):
    """one call of kmpc_lane_step_fleet -> dict v_out [B], gap [B], v_lead [B], leader [B], bound [B], safe_arm [B] (the cap is the sqrt arm's
    value), at [B], winners [B,5] (own-ahead, left-ahead, left-behind, right-ahead, right-behind; -1 = none), nbr [B,4,2], occ [B] uint32,
    rec [B,16] (a new array), moved [B] (+1 left, -1 right, 0)"""
    s, e_ct, v, v_cap = (np.asarray(a, dtype=np.float64) for a in (s, e_ct, v, v_cap))
    fr, lr = np.asarray(follow_rows, dtype=np.float64), np.asarray(lane_rows, dtype=np.float64)
    occ_in = np.asarray(occ_in).astype(np.uint32)
    B = len(s)
    rec = np.array(rec, dtype=np.float64)
    pid = np.zeros(B, dtype=np.int64) if path_id is None else np.asarray(path_id, dtype=np.int64)
    ok = FR.usable(s, v, path_id, present)
    idx = np.arange(B)
    out = dict(v_out=v_cap.copy(), gap=np.full(B, np.inf), v_lead=np.zeros(B), leader=np.full(B, -1, dtype=np.int64), bound=np.zeros(B, dtype=bool),
               safe_arm=np.zeros(B, dtype=bool), at=np.zeros(B), winners=np.full((B, 5), -1, dtype=np.int64), nbr=np.zeros((B, 4, 2)),
               occ=occ_in.copy(), moved=np.zeros(B, dtype=np.int64))
    out["nbr"][:, :, 0] = np.inf
    rec[:, N] += 1.0
    with np.errstate(all="ignore"):
        for b in range(B):
            if not ok[b]:
                continue
            n_lanes, width, v_lat, gain, hold, clear_tol, keep_right = lr[b, 0:7]
            d_min, t_h, a_b, k_gap, length = fr[b, 0:5]
            lane, frm, offset, hold_left = rec[b, LANE], rec[b, LANE_FROM], rec[b, OFFSET], rec[b, HOLD_LEFT]
            # 1: release
            if frm != lane and offset == lane * width and abs(e_ct[b] - offset) <= clear_tol:
                frm = lane
            # 2: the five searches
            has_left, has_right = bool(lane + 1.0 < n_lanes), bool(lane >= 1.0)
            own = bit(lane) | bit(frm)
            lbit = bit(lane + 1.0) if has_left else np.uint32(0)
            rbit = bit(lane - 1.0) if has_right else np.uint32(0)
            cand = ok & (pid == pid[b])
            ahead = cand & ((s > s[b]) | ((s == s[b]) & (idx < b)))
            behind = cand & ((s < s[b]) | ((s == s[b]) & (idx > b)))
            ad = np.abs(s - s[b])
            win, dif = [], []
            for mask, band in ((ahead, own), (ahead, lbit), (behind, lbit), (ahead, rbit), (behind, rbit)):
                d = np.where(mask & ((occ_in & band) != 0), ad, np.inf)
                j = int(np.argmin(d))
                win.append(j if d[j] < np.inf else -1)
                dif.append(d[j])
            out["winners"][b] = win
            # 3: the law on the own-ahead winner
            cap, v_b = v_cap[b], v[b]
            at = a_b * t_h
            out["at"][b] = at
            v_own, bound = cap, False
            if win[0] >= 0:
                o = _side_law(dif[0], v_b, v[win[0]], fr[b], cap)
                v_own, bound = o["v_out"], bool(o["bound"])
                out["gap"][b], out["v_lead"][b], out["leader"][b], out["bound"][b] = o["gap"], v[win[0]], win[0], bound
                out["safe_arm"][b] = bound and not (o["v_gap"] < o["v_safe"]) and o["v_safe"] > 0.0
                rec[b, N_LEADER] += 1.0
                rec[b, N_BOUND] += bound
                rec[b, N_CONTACT] += o["gap"] < 0.0
                rec[b, MIN_GAP] = o["gap"] if o["gap"] < rec[b, MIN_GAP] else rec[b, MIN_GAP]
                c = v_b - v[win[0]]
                rec[b, MAX_CLOSING] = c if c > rec[b, MAX_CLOSING] else rec[b, MAX_CLOSING]
            out["v_out"][b] = v_own
            # 4: the sides and the decision
            lhs_front = (v_b + at) * (v_b + at)
            v_side, safe = [cap, cap], [True, True]
            for side in (0, 1):
                qa, qr = 1 + 2 * side, 2 + 2 * side
                sf = sr = True
                if win[qa] >= 0:
                    v_a = v[win[qa]]
                    o = _side_law(dif[qa], v_b, v_a, fr[b], cap)
                    v_side[side] = o["v_out"]
                    sf = bool(o["gap"] >= d_min) and bool(lhs_front <= o["rad"])
                    out["nbr"][b, 2 * side] = (o["gap"], v_a)
                if win[qr] >= 0:
                    v_r = v[win[qr]]
                    gap_r = dif[qr] - length
                    g = gap_r - d_min
                    gp = g if g > 0.0 else 0.0
                    rad = (at * at + v_b * v_b) + (2.0 * a_b) * gp
                    sr = bool(gap_r >= d_min) and bool((v_r + at) * (v_r + at) <= rad)
                    out["nbr"][b, 2 * side + 1] = (gap_r, v_r)
                safe[side] = sf and sr
            decide = bool(frm == lane) and bool(hold_left == 0.0) and bool(n_lanes > 1.0)
            even = k % 2 == 0
            go_left = decide and has_left and even and bound and bool(v_side[0] - v_own >= gain) and safe[0]
            go_right = decide and has_right and (not even) and bool(keep_right != 0.0) and bool(v_side[1] >= v_own) and safe[1]
            if go_left or go_right:
                frm, lane = lane, (lane + 1.0 if go_left else lane - 1.0)
                hold_left = hold
                rec[b, N_CHANGES] += 1.0
                out["moved"][b] = 1 if go_left else -1
            else:
                h = hold_left - 1.0
                hold_left = h if h > 0.0 else 0.0
            # 5: the ramp; 6: the error against the offset in force before it
            target, stp = lane * width, v_lat * dt
            t = target - offset
            new_offset = target if abs(t) <= stp else (offset + stp if t > 0.0 else offset - stp)
            e = e_ct[b] - offset
            if np.isfinite(e):
                rec[b, SUM_ELANE2] += e * e
                rec[b, MAX_ELANE] = abs(e) if abs(e) > rec[b, MAX_ELANE] else rec[b, MAX_ELANE]
            rec[b, LANE], rec[b, LANE_FROM], rec[b, OFFSET], rec[b, HOLD_LEFT] = lane, frm, new_offset, hold_left
            out["occ"][b] = bit(lane) | bit(frm)
    out["rec"] = rec
    return out


def ref_offset(ref, offset):
    """kmpc_ref_offset_batch: ref [B,H1,3], offset [B] -> a new table; rows with offset 0 keep their bits"""
    ref = np.array(ref, dtype=np.float64)
    d = np.asarray(offset, dtype=np.float64)[:, None]
    out = ref.copy()
    out[:, :, 0] = ref[:, :, 0] - d * np.sin(ref[:, :, 2])
    out[:, :, 1] = ref[:, :, 1] + d * np.cos(ref[:, :, 2])
    keep = np.asarray(offset) == 0.0
    out[keep] = ref[keep]
    return out


# ---------------------------------------------------------------- the seeded draws shared by the CPU and the GPU tests
SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049)     # wave and tile edges: 64 followers per workgroup, 1024 candidates per tile


def draw(B, seed=0, paths=3, bad=True):
    """follow_ref.draw(B, seed, paths, bad) extended with lanes: n_lanes in 1 ... 4 (random rows: width U(3, 4), v_lat U(0.5, 2), gain U(0, 1), hold
    in 0 ... 3, clear_tol U(0.2, 0.8), keep_right 0 / 1, word 7 junk), lanes in 0 ... n_lanes - 1, about 10 % of the vehicles in mid-change (LANE_FROM
    a neighbour of LANE, the offset somewhere on the ramp -- or, for a third of them, already on the target's own bits so that the release can
    happen), about 30 % with HOLD_LEFT > 0, s stretched by max(1, B // 32), e_ct within 0.7 m of the offset; with bad=True about 2 % NaN / inf in e_ct and 1 % junk in a record's
    lane words or a lane row.  -> follow_ref.draw's dict with `follow_rows` for its rows, plus e_ct, lane_rows, rec [B,16], occ (uint32, consistent
    with rec), dt"""
    d = FR.draw(B, seed=seed, paths=paths, bad=bad)
    d["s"] = d["s"] * max(1, B // 32)     # the road grows with the fleet (exactly: ties stay ties), so that gaps stay long enough for safe changes
    rng = np.random.default_rng(77000 * B + seed + 13)
    lr = np.tile(DEFAULT_ROW, (B, 1))
    lr[:, 0] = rng.integers(1, 5, B)
    lr[:, 1], lr[:, 2], lr[:, 3] = rng.uniform(3.0, 4.0, B), rng.uniform(0.5, 2.0, B), rng.uniform(0.0, 1.0, B)
    lr[:, 4], lr[:, 5], lr[:, 6], lr[:, 7] = rng.integers(0, 4, B), rng.uniform(0.2, 0.8, B), rng.integers(0, 2, B), rng.uniform(-9, 9, B)
    lane = np.floor(rng.random(B) * lr[:, 0])
    rec = fresh_rec(B)
    rec[:, LANE] = rec[:, LANE_FROM] = lane
    rec[:, OFFSET] = lane * lr[:, 1]
    mid = (rng.random(B) < 0.10) & (lr[:, 0] > 1)
    dirn = np.where(lane == 0, 1.0, np.where(lane == lr[:, 0] - 1, -1.0, rng.choice([-1.0, 1.0], B)))
    rec[mid, LANE_FROM] = (lane + dirn)[mid]
    on_ramp = mid & (rng.random(B) < 0.67)
    rec[on_ramp, OFFSET] = (lane * lr[:, 1] + dirn * lr[:, 1] * rng.uniform(0.05, 1.0, B))[on_ramp]
    rec[:, HOLD_LEFT] = np.where(rng.random(B) < 0.3, rng.integers(1, 4, B), 0).astype(np.float64)
    rec[:, N_CHANGES] = rng.integers(0, 3, B)
    rec[:, 13:16] = rng.uniform(-9, 9, (B, 3))
    e_ct = rec[:, OFFSET] + rng.uniform(-0.7, 0.7, B)
    if bad:
        junk = np.array([np.nan, np.inf, -np.inf])
        hit = rng.random(B) < 0.02
        e_ct[hit] = junk[rng.integers(0, 3, int(hit.sum()))]
        hit = rng.random(B) < 0.01
        rec[hit, rng.integers(0, 4, int(hit.sum()))] = junk[rng.integers(0, 3, int(hit.sum()))]
        hit = rng.random(B) < 0.01
        lr[hit, rng.integers(0, 7, int(hit.sum()))] = np.array([np.nan, np.inf, -1.0, 40.0])[rng.integers(0, 4, int(hit.sum()))]
    occ = bit(rec[:, LANE]) | bit(rec[:, LANE_FROM])
    out = dict(d, follow_rows=d["rows"], e_ct=e_ct, lane_rows=lr, rec=rec, occ=occ, dt=0.1)
    del out["rows"]
    return out


def step_draw(d, k, occ=None, rec=None):
    """step() on a draw's words (occ and rec of an earlier call in place of the draw's own)"""
    return step(d["s"], d["e_ct"], d["v"], d["path_id"], d["present"], d["follow_rows"], d["lane_rows"], d["v_cap"], d["occ"] if occ is None else occ,
                d["rec"] if rec is None else rec, k, d["dt"])


def calls(B, paths, n=3):
    """n consecutive calls k = 0 ... n-1 on ONE record with ping-ponged occupancy: the rows, record and occupancy of draw(B, 0, paths) to begin with;
    call k sees draw(B, k, paths)'s s, speed, path ids, present and v_cap, and e_ct = the running record's offset + that draw's own deviation from
    its offset (so that releases happen in later calls too).  -> list of (inputs of the call: a draw's dict with the running rec and occ, step()'s
    dict for it)"""
    d0 = draw(B, 0, paths)
    rec, occ, out = d0["rec"], d0["occ"], []
    for k in range(n):
        dk = draw(B, k, paths)
        with np.errstate(invalid="ignore"):
            e_ct = rec[:, OFFSET] + (dk["e_ct"] - dk["rec"][:, OFFSET])
        d = dict(dk, follow_rows=d0["follow_rows"], lane_rows=d0["lane_rows"], e_ct=e_ct, rec=rec, occ=occ)
        e = step_draw(d, k)
        out.append((d, e))
        rec, occ = e["rec"], e["occ"]
    return out


# ---------------------------------------------------------------- the CPU overtaking loop
OVERTAKE = dict(path=0, spacing=20.0, targets=(3.0, 6.0, 6.0), n_lanes=2, steps=400)   # follow_ref.CASES["path1"]'s fleet on two lanes


def cpu_overtake(O, traj, start, targets, follow_rows, lane_rows, steps, weights=None):
    """follow_ref.cpu_platoon with the lane stage in the follower's place: per period the truth's s_along and e_ct (the track score's restatement)
    and speeds -> step() with v_cap = targets, k the period's index, dt = N_UPD x 10 ms -> per vehicle the oracle's waypoints at the stage's cap,
    shifted by the vehicle's new offset (ref_offset), and the condensed solver -> road_ref's plant.
    -> dict state [steps+1,B,8], cmd, status, v_follow, gap, leader, lane, lane_offset [steps,B], rec [B,16], stop, s_along [B] of the last state"""
    from oracle import waypoints as W, vehicle_sim as Vs
    import scenario as S
    B = len(start)
    targets = np.asarray(targets, dtype=np.float64)
    p = O.params(8, weights if weights is not None else S.WEIGHTS)
    s = np.concatenate([Vs.initial_state(1, traj[i, 4], traj[i, 5], traj[i, 3]) for i in start])
    s[:, 3] = targets
    plant, road = np.tile(R.DEFAULT_ROW, (B, 1)), np.tile(RR.NEUTRAL_ROW, (B, 1))
    u_prev, U_prev, have_warm = np.zeros((B, 2)), [None] * B, False
    cmds, states = np.zeros((steps, B, 2)), np.zeros((steps + 1, B, 8))
    status = np.zeros((steps, B), dtype=np.int64)
    v_follow, gap, lane, lane_offset = (np.zeros((steps, B)) for _ in range(4))
    leader = np.zeros((steps, B), dtype=np.int64)
    states[0] = s
    pstat, near, stop_any = np.zeros((B, 4)), np.zeros(B, dtype=bool), False
    rec, occ = fresh_rec(B), np.ones(B, dtype=np.uint32)
    for k in range(steps):
        e = TS.errors(traj, s[:, 0], s[:, 1], s[:, 2])
        f = step(e["s_along"], e["e_ct"], s[:, 3], None, None, follow_rows, lane_rows, targets, occ, rec, k, 0.01 * FR.N_UPD)
        rec, occ = f["rec"], f["occ"]
        v_follow[k], gap[k], leader[k], lane[k], lane_offset[k] = f["v_out"], f["gap"], f["leader"], rec[:, LANE], rec[:, OFFSET]
        for b in range(B):
            x, y, psi, v = s[b, 0:4]
            xr, yr, pr, stop, _ci = W.get_waypoints(traj, x, y, psi, v_follow[k, b], traj_horizon=8)
            stop_any |= bool(stop)
            ref = ref_offset(np.stack([xr, yr, pr], 1)[None], rec[b:b + 1, OFFSET])[0]
            q = O.problem(p, [x, y, psi, v], ref, v_follow[k, b], u_prev[b])
            r = O.solve_condensed(p, q, o=O.opts(warm=1) if have_warm else O.opts(), U0=U_prev[b])
            cmds[k, b] = r["U"][0]
            u_prev[b], U_prev[b] = r["U"][0].copy(), r["U"].copy()
            status[k, b] = r["status"]
        have_warm = True
        s, pstat = RR.advance_road(s, cmds, k, plant, road, [0] * B, 2, FR.N_UPD, stat=pstat, near=near)
        states[k + 1] = s
    return dict(state=states, cmd=cmds, status=status, v_follow=v_follow, gap=gap, leader=leader, lane=lane, lane_offset=lane_offset, rec=rec,
                stop=stop_any, s_along=TS.errors(traj, s[:, 0], s[:, 1], s[:, 2])["s_along"])


_cache = {}


def cached_overtake(O, n_lanes=2, steps=None):
    """OVERTAKE on n_lanes lanes, computed once per process -> (cpu_overtake's dict, trajectory, start indices)"""
    import fleet_scenario as F
    c = OVERTAKE
    steps = c["steps"] if steps is None else steps
    tr = F.trajectory(c["path"])
    B = len(c["targets"])
    start = FR.platoon_start(tr, c["spacing"], B)
    key = (n_lanes, steps)
    if key not in _cache:
        _cache[key] = cpu_overtake(O, tr, start, c["targets"], FR.rows(B), rows(B, n_lanes=n_lanes), steps)
    return _cache[key], tr, start
