"""The range sensor and leader tracker on the device: kmpc_range_follow_batch against the numpy restatement tests/range_ref.py on seeded draws,
behind kmpc_follow_fleet through ref_traj.Follower(radar=), and inside the closed loops.

Tolerances.  Without noise every word is exact: the draws' dropout word is integer arithmetic, the filter is correctly rounded +, -, x and /
in one order, and v_cap_out is exact except where the Gipps arm gave it, which passes through the device's fp64 sqrt: tests/test_follow.py's
allowance of 2 ulp of the square-root term (measured: MEASURED_SQRT_ULP).  With noise the two normals come from the device's log / sqrt / cos /
sin: range_ref.TOL_N = 1e-13 per normal (tests/test_plant_sensor.py's bound), and everything downstream follows range_ref.bounds, which is
derived there line by line: P, the gains, the counters, the track id and COAST are functions of the rows, the truth and integer draws -- exact;
GAP_HAT, V_HAT, v_cap_out and the two error words carry the measurement's allowance through the restatement's own (exact) gains, dt coupling
the speed error into the gap.  The loop against the CPU loop: tests/test_road.py's TOL_LOOP."""
import numpy as np
import pytest

import fleet_scenario as F
import follow_ref as FR
import range_ref as RG

pytestmark = pytest.mark.gpu

# measured on the MI355X: the largest distance of a Gipps-arm cap from the restatement's, in ulp of the square-root term, over every draw of
# test_noise_free_parity
MEASURED_SQRT_ULP = 0
# measured on the MI355X: the largest ratio of a deviation to its derived bound over every draw of test_noisy_parity (z_r, z_v, GAP_HAT, V_HAT,
# v_cap_out, SUM_EGAP2, MAX_EGAP), and the number of vehicles whose N_BOUND was excused
MEASURED_NOISY_RATIO = 0.094
MEASURED_NOISY_EXCUSED = 0
# measured on the MI355X: the three-vehicle path1 platoon with a noise-free, non-neutral radar against the CPU loop, largest position difference [m]
# and largest difference of the other states and the commands
MEASURED_LOOP = (2.930e-14, 6.543e-14)
TOL_LOOP = np.array([4.8e-10, 4.9e-9])     # tests/test_road.py's TOL_LOOP
LOOP_ROW = dict(sigma_r=0.0, sigma_v=0.0, bias_r=0.3, range_max=40.0, p_drop=0.2, filter=1.0)
NOISY_ROW = dict(sigma_r=0.5, p_drop=0.2, filter=1.0)
SEED, PERIOD0 = 5, 11


def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64).cuda()


def same_bits(a, b):
    """the same 64-bit patterns; a NaN matches a NaN (an arithmetic NaN's sign and payload are the processor's, not the stage's)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()


class Stage:
    """the buffers of one fleet's stage: the speeds inside [B,8] and [B,4] tables at column 3, as the loops hand them over; the outputs start as
    7.0, so a word nobody wrote shows"""

    def __init__(self, d, sl=slice(None), rec=None, same_speed=False, inplace=False, want_meas=True):
        import torch
        self.d, self.sl, self.same_speed, self.inplace = d, sl, same_speed, inplace
        self.B = len(d["v_cap"][sl])
        self.frows, self.rrows = dev(d["follow_rows"][sl]), dev(d["range_rows"][sl])
        self.rec = dev(RG.fresh_rec(self.B) if rec is None else rec)
        self.meas = torch.full((self.B, 4), 7.0, dtype=torch.float64, device="cuda") if want_meas else None

    def call(self, c, seed=SEED, period=None, id_base=0):
        """call c of the draw -> v_cap_out as numpy"""
        import torch
        from mkz_mpc_path_follower_amd import _lib
        from mkz_mpc_path_follower_amd._stage import ptr, stream
        d, sl, B = self.d, self.sl, self.B
        state, known = np.full((B, 8), -7.0), np.full((B, 4), -7.0)
        state[:, 3], known[:, 3] = d["v_true"][c][sl], d["v_known"][c][sl]
        state, known = dev(state), dev(known)
        truth, leader, cap = dev(d["truth"][c][sl]), dev(d["leader"][c][sl], torch.int32), dev(d["v_cap"][sl])
        out = cap if self.inplace else torch.full((B,), 7.0, dtype=torch.float64, device="cuda")
        vk, ks = (state[:, 3], 8) if self.same_speed else (known[:, 3], 4)
        _lib.check(_lib.load().kmpc_range_follow_batch(0, B, RG.DT, ptr(truth), ptr(leader), ptr(state[:, 3]), 8, ptr(vk), ks, ptr(self.frows),
                                                       ptr(self.rrows), seed, PERIOD0 + c if period is None else period, id_base, ptr(cap),
                                                       ptr(out), ptr(self.rec), ptr(self.meas), stream(torch.device("cuda", 0))))
        torch.cuda.synchronize()
        return out.cpu().numpy()


EXACT_WORDS = [RG.P00, RG.P01, RG.P11, RG.TRACK_ID, RG.COAST, RG.N, RG.N_DETECT, RG.N_DROP, RG.N_OUT, RG.N_NEW, RG.N_LOST]


def sqrt_ulp(v_out, e, what):
    """v_cap_out exact off the Gipps arm, within 2 ulp of the square-root term on it -> the largest such deviation [ulp]"""
    exact = ~e["safe_arm"]
    assert same_bits(v_out[exact], e["v_out"][exact]), (what, np.flatnonzero(exact & (v_out != e["v_out"]))[:8])
    if not e["safe_arm"].any():
        return 0.0
    f = np.flatnonzero(e["safe_arm"])
    dev_ulp = np.abs(v_out[f] - e["v_out"][f]) / np.spacing(e["v_out"][f] + e["at"][f])     # sqrt(rad) = v_safe + at
    assert (dev_ulp <= 2.0).all(), (what, dev_ulp.max())
    return float(dev_ulp.max())


# ---------------------------------------------------------------- 1: noise-free parity
@pytest.mark.parametrize("B", RG.SIZES)
def test_noise_free_parity(B):
    """range_ref.draw(noisy=False) at the block and wave edges, three consecutive calls on one record: sigmas 0, but bias, range limits, P_DROP 0 or
    0.3, FILTER 0 / 1 mixed, coasting, leader changes, 5 % without a leader and 5 % non-finite inputs.  Exact: every word of the record, meas_out,
    and v_cap_out off the Gipps arm; on it within 2 ulp of the square-root term.
    Measured on the MI355X: MEASURED_SQRT_ULP ulp at most (the device's fp64 sqrt rounded as numpy's)."""
    worst, n_safe = 0.0, 0
    for seed in (0, 1):
        d = RG.draw(B, seed, noisy=False)
        ref = RG.run(d, seed=SEED, period0=PERIOD0)
        st = Stage(d)
        for c, e in enumerate(ref):
            v_out = st.call(c)
            worst = max(worst, sqrt_ulp(v_out, e, (B, seed, c)))
            n_safe += int(e["safe_arm"].sum())
            rec, meas = st.rec.cpu().numpy(), st.meas.cpu().numpy()
            for w in range(16):
                assert same_bits(rec[:, w], e["rec"][:, w]), (B, seed, c, RG.REC_FIELDS[w], np.flatnonzero(rec[:, w] != e["rec"][:, w])[:8])
            assert same_bits(meas, e["meas"]), (B, seed, c)
        assert (ref[-1]["rec"][:, RG.N] == 3.0).all()
    print("B = %d: %d Gipps-arm caps, largest deviation %.2f ulp of the square-root term" % (B, n_safe, worst))


# ---------------------------------------------------------------- 2: noisy parity
@pytest.mark.parametrize("B", RG.SIZES)
def test_noisy_parity(B):
    """range_ref.draw at the same sizes, three calls from a fresh record.  z_r and z_v within TOL_N * sigma plus one ulp of the sum; GAP_HAT, V_HAT,
    v_cap_out, SUM_EGAP2 and MAX_EGAP within range_ref.bounds (derived there: a new track or FILTER = 0 carries the measurement's allowance; the
    prediction adds dt times the speed's; each scalar update mixes state and measurement allowances with the restatement's own gains, which are
    exact because P never sees a measurement; the law is 1-Lipschitz in its arms, the square root at worst min(d / sqrt(x), sqrt(d)); eight ulp
    for correctly rounded operations on inputs that differ).  P, TRACK_ID, COAST and the counters N, N_DETECT, N_DROP, N_OUT, N_NEW, N_LOST:
    exact.  N_BOUND may differ only for vehicles whose restated |v_f - v_cap| lies within the bound on v_cap_out, and for at most 1 % of a draw.
    Measured on the MI355X: largest ratio of a deviation to its bound MEASURED_NOISY_RATIO; MEASURED_NOISY_EXCUSED vehicles excused."""
    worst, excused_all = 0.0, 0
    for seed in (0, 1):
        d = RG.draw(B, seed)
        ref = RG.run(d, seed=SEED, period0=PERIOD0)
        bnd = RG.bounds(d["follow_rows"], d["range_rows"], ref, RG.DT)
        st = Stage(d)
        excused = np.zeros(B, dtype=bool)
        for c, (e, b) in enumerate(zip(ref, bnd)):
            v_out = st.call(c)
            rec, meas = st.rec.cpu().numpy(), st.meas.cpu().numpy()
            for w in EXACT_WORDS:
                assert same_bits(rec[:, w], e["rec"][:, w]), (B, seed, c, RG.REC_FIELDS[w])
            assert same_bits(meas[:, 2:4], e["meas"][:, 2:4]), (B, seed, c)
            pairs = (("z_r", meas[:, 0], e["meas"][:, 0]), ("z_v", meas[:, 1], e["meas"][:, 1]), ("gap_hat", rec[:, 0], e["rec"][:, 0]),
                     ("v_hat", rec[:, 1], e["rec"][:, 1]), ("v_out", v_out, e["v_out"]), ("sum_egap2", rec[:, 14], e["rec"][:, 14]),
                     ("max_egap", rec[:, 15], e["rec"][:, 15]))
            for name, got, want in pairs:
                fin = np.isfinite(want)
                assert same_bits(got[~fin], want[~fin]), (B, seed, c, name)
                diff = np.abs(got[fin] - want[fin])
                assert (diff <= b[name][fin]).all(), (B, seed, c, name, float((diff / b[name][fin])[diff > 0].max()))
                if (diff > 0).any():
                    worst = max(worst, float((diff[diff > 0] / b[name][fin][diff > 0]).max()))
            excused |= e["margin"] <= b["v_out"]
            assert np.array_equal(rec[~excused, RG.N_BOUND], e["rec"][~excused, RG.N_BOUND]), (B, seed, c)
        assert excused.sum() <= 0.01 * B, (B, seed, int(excused.sum()))
        excused_all += int(excused.sum())
    print("B = %d: largest deviation / bound %.3f, %d vehicles' N_BOUND excused" % (B, worst, excused_all))


# ---------------------------------------------------------------- 3: the chain behind kmpc_follow_fleet
def _fleet_on_three_paths(B, seed):
    """B vehicles on recorded samples of the three fixture paths at the samples' headings, speeds U(0, 10) -> (path ids, state [B,8])"""
    rng = np.random.default_rng(seed)
    pid = rng.integers(0, 3, B).astype(np.int32)
    state = np.zeros((B, 8))
    for p in range(3):
        tr = F.trajectory(p)
        i = rng.integers(20, len(tr) - 20, int((pid == p).sum()))
        state[pid == p, 0], state[pid == p, 1], state[pid == p, 2] = tr[i, 4], tr[i, 5], tr[i, 3]
    state[:, 3] = rng.uniform(0.0, 10.0, B)
    return pid, state


def test_neutral_radar_and_plain_follower_give_the_same_bits():
    """B = 257 on three paths, three calls with fresh speeds: Follower with the neutral radar against Follower without -- cap() outputs, gap, leader
    and stat bit for bit, v_ideal the same bits again, gap_seen = gap; and a Follower without radar= against the hand-made kmpc_follow_fleet call"""
    import torch
    from mkz_mpc_path_follower_amd import FleetRefTrajectory, _lib
    from mkz_mpc_path_follower_amd._stage import ptr, stream
    from mkz_mpc_path_follower_amd.ref_traj import Follower, RangeSensor, follow_params, fresh_follow_stat, range_neutral
    B = 257
    pid, state = _fleet_on_three_paths(B, 21)
    grt = FleetRefTrajectory([F.path_dict(p) for p in range(3)], pid, traj_horizon=8, traj_dt=0.2)
    rows = FR.draw(B, 0, paths=0, bad=False)["rows"]
    radar = RangeSensor(B, rows=dev(np.tile(range_neutral(), (B, 1))), seed=9)
    plain, seen = Follower(grt, rows=dev(rows)), Follower(grt, rows=dev(rows), radar=radar)
    assert plain.radar is None and plain.v_ideal is None and seen.radar is radar
    with pytest.raises(ValueError, match="k="):
        seen.cap(dev(state), dev(np.full(B, 9.0)))
    with pytest.raises(ValueError, match="radar"):
        plain.cap(dev(state), dev(np.full(B, 9.0)), k=0, dt=0.1)
    with pytest.raises(ValueError, match="radar"):
        plain.gap_seen
    with pytest.raises(ValueError):
        Follower(grt, rows=dev(rows), radar=RangeSensor(B - 1))
    cap = dev(np.random.default_rng(4).uniform(2.0, 12.0, B))
    stat, gl, ld = fresh_follow_stat(B, torch.device("cuda", 0)), torch.empty((B, 2), dtype=torch.float64, device="cuda"), torch.empty((B,), dtype=torch.int32, device="cuda")
    n_lead = 0
    for k in range(3):
        state[:, 3] = np.random.default_rng(30 + k).uniform(0.0, 10.0, B)
        st = dev(state)
        a, b = plain.cap(st, cap), seen.cap(st, cap, k=k, dt=0.1)
        hand = torch.empty((B,), dtype=torch.float64, device="cuda")
        _lib.check(_lib.load().kmpc_follow_fleet(0, B, ptr(plain._track["err"][:, 3]), 4, ptr(st[:, 3]), 8, ptr(grt.path_id), ptr(plain._on_path),
                                                 ptr(plain.rows), ptr(cap), ptr(hand), ptr(gl), ptr(ld), ptr(stat), stream(torch.device("cuda", 0))))
        torch.cuda.synchronize()
        assert same_bits(a.cpu().numpy(), b.cpu().numpy()) and same_bits(a.cpu().numpy(), hand.cpu().numpy()), k
        assert same_bits(seen.v_ideal.cpu().numpy(), a.cpu().numpy())
        for x, y, z in ((plain.gap_leader, seen.gap_leader, gl), (plain.stat, seen.stat, stat)):
            assert same_bits(x.cpu().numpy(), y.cpu().numpy()) and same_bits(x.cpu().numpy(), z.cpu().numpy()), k
        assert torch.equal(plain.leader, seen.leader) and torch.equal(plain.leader, ld)
        assert same_bits(seen.gap_seen.cpu().numpy(), plain.gap.cpu().numpy()) and same_bits(seen.v_lead_seen.cpu().numpy(), plain.leader_speed.cpu().numpy())
        n_lead += int((ld >= 0).sum().item())
    s = radar.summary()
    assert n_lead > 600 and (s["n"] == 3).all() and s["n_detect"].sum() == n_lead and s["n_drop"].sum() == 0 and (s["max_egap"] == 0.0).all()
    seen.reset()
    assert same_bits(radar.rec.cpu().numpy(), RG.fresh_rec(B))


def _platoon_loop(radar_rows, cls=None, steps=150, seed=0, **kw):
    """follow_ref.CASES["path1"] in one loop on a one-path fleet, on the neutral road, with Follower(radar=) for rows given (None: no radar)
    -> (loop, run()'s dict as numpy)"""
    import torch
    from mkz_mpc_path_follower_amd import FleetRefTrajectory
    from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop
    from mkz_mpc_path_follower_amd.ref_traj import Follower, RangeSensor, follow_params
    from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator, road_params
    c = FR.CASES["path1"]
    targets = list(c["targets"])
    B = len(targets)
    tr = F.trajectory(c["path"])
    start = FR.platoon_start(tr, c["spacing"], B)
    grt = FleetRefTrajectory([F.path_dict(c["path"])], [0] * B, traj_horizon=8, traj_dt=0.2)
    sim = VehicleSimulator(B, X0=tr[start, 4], Y0=tr[start, 5], Psi0=tr[start, 3], road=road_params(B))
    sim.state[:, 3] = torch.as_tensor(targets, dtype=torch.float64, device=sim.device)
    radar = None if radar_rows is None else RangeSensor(B, rows=dev(radar_rows), seed=seed)
    loop = (cls or ClosedLoop)(grt, sim, N=8, target_vel=targets, follower=Follower(grt, rows=follow_params(B, **c["row"]), radar=radar), **kw)
    out = loop.run(steps, history=True)
    torch.cuda.synchronize()
    return loop, {k: v.cpu().numpy() for k, v in out.items() if isinstance(v, torch.Tensor)}


@pytest.mark.parametrize("frenet", [False, True])
def test_neutral_radar_leaves_the_platoon_loop_bit_for_bit(frenet):
    """the three-vehicle, 150-period platoon with the neutral radar: state, command, v_follow and gap histories (status, latch and score too) bit for
    bit those of follower= alone; gap_seen and v_lead_seen are the truth's"""
    from mkz_mpc_path_follower_amd.closed_loop import ClosedLoopFrenet
    cls = ClosedLoopFrenet if frenet else None
    _, a = _platoon_loop(None, cls)
    loop, b = _platoon_loop(RG.neutral_rows(3), cls)
    assert "gap_seen" not in a and b["gap_seen"].shape == b["v_lead_seen"].shape == (150, 3)
    for k in ("state", "cmd", "v_follow", "gap", "score"):
        assert same_bits(a[k], b[k]), k
    assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["latch"], b["latch"])
    assert same_bits(b["gap_seen"], b["gap"]) and (b["v_lead_seen"][:, 0] == 0.0).all()
    assert loop.follower.radar.summary()["n_detect"].tolist() == [0, 150, 150]


# ---------------------------------------------------------------- 4: the loop against the CPU loop
def test_loop_matches_the_cpu_platoon(oracle):
    """the path1 platoon with a noise-free but non-neutral radar (bias 0.3 m, RANGE_MAX = 40 m, P_DROP = 0.2, FILTER = 1), 150 periods in ONE
    ClosedLoop against range_ref.cpu_platoon: states and commands within tests/test_road.py's TOL_LOOP, identical detection histories, every
    solve Optimal, no contact.  Measured on the MI355X: 2.930e-14 m on positions, 6.543e-14 on the other states and the commands (MEASURED_LOOP);
    v_follow within 1.7e-14 m/s and the tracked gaps within 2.7e-14 m of the CPU loop's; 33 and 27 dropped periods of 150, nobody out of range."""
    rr = RG.rows(3, **LOOP_ROW)
    r, _, _ = RG.cached_platoon(oracle, "path1", "loop_row", rr)
    loop, g = _platoon_loop(rr)
    assert (g["status"] == 0).all() and not g["latch"].any() and np.isfinite(g["state"]).all() and (r["status"] == 0).all()
    s, rs = loop.follower.summary(), loop.follower.radar.summary()
    assert (s["n_contact"] == 0).all() and (g["gap"] >= 0.0).all() and (rs["n"] == 150).all()
    for k, w in (("n_detect", RG.N_DETECT), ("n_drop", RG.N_DROP), ("n_out", RG.N_OUT), ("n_new", RG.N_NEW), ("n_lost", RG.N_LOST)):
        assert rs[k].tolist() == r["rec"][:, w].astype(int).tolist(), k
    assert np.array_equal(np.isposinf(g["gap_seen"]), np.isposinf(r["gap_seen"]))          # a track in the same periods
    assert rs["n_drop"][1:].min() > 10
    dp = np.hypot(g["state"][:, :, 0] - r["state"][:, :, 0], g["state"][:, :, 1] - r["state"][:, :, 1]).max()
    do = max(np.abs(g["state"][:, :, 2:] - r["state"][:, :, 2:]).max(), np.abs(g["cmd"] - r["cmd"]).max())
    tr = np.isfinite(r["gap_seen"])
    dv, dg = np.abs(g["v_follow"] - r["v_follow"]).max(), np.abs(g["gap_seen"][tr] - r["gap_seen"][tr]).max()
    print("radar platoon against the CPU loop: max |dpos| %.3e m, other states and commands %.3e (bounds %s); v_follow %.3e m/s, gap_seen %.3e m; "
          "smallest gap %s m; detections %s, drops %s, out of range %s" % (dp, do, TOL_LOOP, dv, dg, np.round(s["min_gap"], 3), rs["n_detect"].tolist(),
                                                                            rs["n_drop"].tolist(), rs["n_out"].tolist()))
    assert dp <= TOL_LOOP[0] and do <= TOL_LOOP[1]


# ---------------------------------------------------------------- 5: the noisy loop
def test_noisy_loop_keeps_its_distance():
    """SIGMA_R = 0.5 m, P_DROP = 0.2, FILTER = 1, with sensor= and estimator= so that the speed the controller knows is not the truth's, stepped
    period by period: every state finite, every solve Optimal, no contact in follower.stat (the truth's record), the radar's counts consistent,
    and each period's meas against the restatement fed that period's truth (the search's gap and leader, the plant's speeds, est_filt's speed):
    detected and COAST exact, z_r and z_v within test 2's TOL_N * sigma plus one ulp of the sum"""
    import torch
    from mkz_mpc_path_follower_amd.vehicle_sim import Estimator, SensorModel
    seed = 17
    rr = RG.rows(3, **NOISY_ROW)
    loop, _ = _platoon_loop(rr, steps=0, seed=seed, sensor=SensorModel(3, sigma=(0.2, 0.2, 0.01, 0.1), seed=7), estimator=Estimator(3))
    fo = loop.follower
    frows, targets, rec = FR.rows(3), np.array(FR.CASES["path1"]["targets"]), RG.fresh_rec(3)
    differs = False
    for k in range(150):
        v = loop.sim.state[:, 3].cpu().numpy()
        o = loop.step()
        torch.cuda.synchronize()
        assert (o["status"] == 0).all().item() and torch.isfinite(loop.sim.state).all().item(), k
        known = loop.est_filt[:, 3].cpu().numpy()
        differs |= bool((known != v).any())
        e = RG.step(fo.gap_leader.cpu().numpy(), fo.leader.cpu().numpy(), v, known, frows, rr, seed, k, 0, targets, rec, 0.1)
        rec = e["rec"]
        meas, det = fo.radar.meas.cpu().numpy(), e["det"]
        assert same_bits(meas[:, 2:4], e["meas"][:, 2:4]) and np.isnan(meas[~det, 0:2]).all(), k
        for c, sigma in ((0, rr[:, 1]), (1, rr[:, 2])):
            tol = RG.TOL_N * sigma[det] + np.spacing(np.abs(e["meas"][det, c]))
            assert (np.abs(meas[det, c] - e["meas"][det, c]) <= tol).all(), (k, c)
        assert np.array_equal(fo.radar.rec[:, RG.TRACK_ID].cpu().numpy(), rec[:, RG.TRACK_ID]), k
        rec[:, 0:2] = fo.radar.rec[:, 0:2].cpu().numpy()      # follow the device's own track: this test is about the measurements
    s, rs = fo.summary(), fo.radar.summary()
    print("noisy loop: smallest true gaps %s m, detections %s, drops %s, rms gap error %s m" % (np.round(s["min_gap"], 3), rs["n_detect"].tolist(),
          rs["n_drop"].tolist(), np.round(np.sqrt(rs["sum_egap2"] / 150.0), 3)))
    assert differs and not loop.command_stop.any().item()
    assert (s["n_contact"] == 0).all() and s["min_gap"][1:].min() > 0.0 and (s["n"] == 150).all()
    assert (rs["n_detect"] + rs["n_drop"] + rs["n_out"] <= rs["n"]).all() and (rs["n"] == 150).all() and rs["n_drop"][1:].min() > 10
    for key, w in (("n_detect", RG.N_DETECT), ("n_drop", RG.N_DROP), ("n_new", RG.N_NEW), ("n_lost", RG.N_LOST)):
        assert rs[key].tolist() == rec[:, w].astype(int).tolist(), key


# ---------------------------------------------------------------- 6: aliasing and optional outputs
def test_aliasing_optional_outputs_and_sharding():
    """v_cap_out aliasing v_cap; meas_out = NULL; speed_known the pointer of speed_true; and two half-fleet calls with id_base equal to one whole-fleet
    call exactly, noise included (two device runs: the same library calls on the same words)"""
    B = 257
    d = RG.draw(B, 3)
    base = Stage(d)
    outs = [base.call(c) for c in range(3)]
    rec, meas = base.rec.cpu().numpy(), base.meas.cpu().numpy()
    for kw in (dict(inplace=True), dict(want_meas=False)):
        st = Stage(d, **kw)
        for c in range(3):
            assert same_bits(st.call(c), outs[c]), (kw, c)
        assert same_bits(st.rec.cpu().numpy(), rec), kw
    lo, hi = Stage(d, slice(0, 100)), Stage(d, slice(100, B))
    for c in range(3):
        assert same_bits(np.concatenate([lo.call(c), hi.call(c, id_base=100)]), outs[c]), c
    assert same_bits(np.concatenate([lo.rec.cpu().numpy(), hi.rec.cpu().numpy()]), rec)
    assert same_bits(np.concatenate([lo.meas.cpu().numpy(), hi.meas.cpu().numpy()]), meas)
    # the same pointer for both speeds: the restatement with v_known = v_true, noise-free, exact off the Gipps arm
    dn = RG.draw(B, 4, noisy=False)
    dn["v_known"] = [v.copy() for v in dn["v_true"]]
    st = Stage(dn, same_speed=True)
    for c, e in enumerate(RG.run(dn, seed=SEED, period0=PERIOD0)):
        sqrt_ulp(st.call(c), e, ("same pointer", c))
        assert same_bits(st.rec.cpu().numpy(), e["rec"]) and same_bits(st.meas.cpu().numpy(), e["meas"]), c
    # B == 0: no launch
    d0 = {k: ([a[:0] for a in v] if isinstance(v, list) else v[:0]) for k, v in d.items()}
    assert Stage(d0).call(0).shape == (0,)
