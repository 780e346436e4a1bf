"""The disturbance observer and the command offset on the device (kmpc_observe_batch, kmpc_cmd_offset_batch, vehicle_sim.DisturbanceObserver, the
loops' `observer=`) against the numpy restatement of tests/observer_ref.py, against kmpc_estimate_batch (the p0 = q_dist = 0 reduction, exact),
against itself (poisoned neighbours) and against a CPU loop made of the oracle's parts.

Tolerances.  Kernel against restatement: same operations in the same order, contraction off; what differs is the device library's tan / atan /
sin / cos / sqrt (a few ulp from numpy's).  The project's rule (tests/test_estimator.py): 10 x the value measured on the MI355X, capped at 1e-9 (m,
rad, m/s, m/s^2; relative to the record's largest covariance word for P); where the measurement is below the smallest difference the quantity can
show (one ulp of x, y = 500 m, 1.137e-13) the bound is 10 x that ulp.  Measured on the MI355X, single call (B = 300): MEASURED_CALL; 100-call
recursion (65 vehicles): MEASURED_RUN; both in the order record state, P (relative), est, dist, innov.  Flags and the two counters are exact.
The loop against the CPU loop: 10 x measured, capped at 1e-6 (tests/test_road.py's loop test: loop drift through a different libm): MEASURED_LOOP."""
import ctypes as C

import numpy as np
import pytest

import estimator_ref as E
import observer_ref as OR
import road_ref as RR
import scenario as S

pytestmark = pytest.mark.gpu

# measured on the MI355X (2026-10-19); bound = 10 x measured, or 10 x the ulp of the column's largest value where the measurement is below that ulp
# (x, y = 500 m: 1.137e-13, so record state and est; a disturbance of order 1: 2.220e-16, so dist of the single call)
MEASURED_CALL = (1.110e-16, 2.251e-16, 1.110e-16, 1.110e-16, 5.509e-15)
TOL_CALL = np.array([1.2e-12, 2.3e-15, 1.2e-12, 2.3e-15, 5.6e-14])
MEASURED_RUN = (2.842e-14, 2.001e-16, 2.842e-14, 1.582e-15, 1.331e-13)
TOL_RUN = np.array([1.2e-12, 2.1e-15, 1.2e-12, 1.6e-14, 1.4e-12])
MEASURED_LOOP = (1.618e-12, 3.110e-11, 1.452e-13)   # positions [m], other states and commands, d-hat: the worst of the six vehicles over 120 periods
TOL_LOOP = np.array([1.7e-11, 3.2e-10, 1.5e-12])


def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64).cuda()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def lib():
    from mkz_mpc_path_follower_amd import _lib
    return _lib.load()


def observe(rec, z, u, params, gate=0.0, dt=0.1, v_min=OR.V_MIN, psi_cap=OR.PSI_CAP):
    """kmpc_observe_batch on a copy of `rec` (numpy in, numpy out) -> rec, est, dist, innov, flags"""
    import torch
    B = len(rec)
    r, zz, uu, pp = dev(rec), dev(z), dev(u), dev(params)
    est = torch.full((B, 4), 777.0, dtype=torch.float64, device="cuda")
    dist = torch.full((B, 3), 777.0, dtype=torch.float64, device="cuda")
    innov = torch.full((B, 4), 777.0, dtype=torch.float64, device="cuda")
    flags = torch.full((B,), 777, dtype=torch.int32, device="cuda")
    assert lib().kmpc_observe_batch(0, B, ptr(r), ptr(zz), ptr(uu), 2, ptr(pp), dt, OR.L_A, OR.L_B, gate, v_min, psi_cap, ptr(est), ptr(dist), ptr(innov),
                                    ptr(flags), None) == 0
    torch.cuda.synchronize()
    return r.cpu().numpy(), est.cpu().numpy(), dist.cpu().numpy(), innov.cpu().numpy(), flags.cpu().numpy()


def errors(rec, exp_rec, est, exp_est, dist, exp_dist, innov, exp_innov):
    """-> [record state, P relative to the record's largest |P| word, est, dist, innov], headings modulo 2 pi"""
    dx = np.abs(rec[..., 0:7] - exp_rec[..., 0:7])
    dx[..., 2] = np.abs(OR.wrap(rec[..., 2] - exp_rec[..., 2]))
    scale = np.maximum(np.abs(exp_rec[..., 7:35]).max(-1, keepdims=True), 1e-300)
    de = np.abs(est - exp_est)
    de[..., 2] = np.abs(OR.wrap(est[..., 2] - exp_est[..., 2]))
    return np.array([dx.max(), (np.abs(rec[..., 7:35] - exp_rec[..., 7:35]) / scale).max(), de.max(), np.abs(dist - exp_dist).max(),
                     np.abs(innov - exp_innov).max()])


def as_numbers(a, b):
    """equal as numbers: a -0 may be a +0, NaN equals NaN"""
    return np.array_equal(np.asarray(a) + 0.0, np.asarray(b) + 0.0, equal_nan=True)


# ---------------------------------------------------------------- 1: one call against the restatement
def test_single_call_matches_the_restatement():
    """tests/observer_ref.py::single_call_case (tests/test_observer_ref.py checks its groups on the CPU): B = 300, two blocks and a partial wave,
    fresh records, dropouts, gated channels, slow vehicles under v_min, d's of both signs.  Flags and both counters exact, the rest within TOL_CALL
    = 10 x MEASURED_CALL (module docstring).
    Measured on the MI355X: record state 1.110e-16, P 2.251e-16 relative, est 1.110e-16, dist 1.110e-16, innov 5.509e-15; bounds 1.2e-12 (10 ulp of
    500 m), 2.3e-15, 1.2e-12, 2.3e-15 (10 ulp of 1), 5.6e-14."""
    c = OR.single_call_case()
    kw = dict(gate=c["gate"], v_min=c["v_min"], psi_cap=c["psi_cap"])
    exp = OR.observe(c["rec"], c["z"], c["u"], c["params"], **kw)
    got = observe(c["rec"], c["z"], c["u"], c["params"], **kw)
    assert np.array_equal(got[4], exp[4])
    assert np.array_equal(got[0][:, OR.COUNT], exp[0][:, OR.COUNT]) and np.array_equal(got[0][:, OR.SKIPPED], exp[0][:, OR.SKIPPED])
    assert not got[0][:, 37:40].any()
    nanz = ~np.isfinite(c["z"]).all(1) & (exp[0][:, OR.COUNT] == 0)
    assert nanz.sum() == 2 and np.array_equal(got[1][nanz], c["z"][nanz], equal_nan=True) and not got[0][nanz].any() and not got[2][nanz].any()
    init = exp[4] == OR.INIT
    assert init.sum() == 8 and np.array_equal(got[1][init], c["z"][init]) and np.array_equal(got[0][init], exp[0][init])
    ok = ~nanz
    err = errors(got[0][ok], exp[0][ok], got[1][ok], exp[1][ok], got[2][ok], exp[2][ok], got[3], exp[3])
    print("single call against numpy: record state %.3e, P %.3e (relative), est %.3e, dist %.3e, innov %.3e" % tuple(err))
    assert np.isfinite(got[0]).all() and np.isfinite(got[3]).all()
    assert (err <= TOL_CALL).all() and TOL_CALL.max() <= 1e-9
    assert np.array_equal(got[2], got[0][:, 4:7])
    # u through a stride, and without the optional outputs: the same bits
    import torch
    st8 = np.zeros((len(c["rec"]), 8)); st8[:, 6:8] = c["u"]
    r2, s8, e2 = dev(c["rec"]), dev(st8), torch.empty((len(c["rec"]), 4), dtype=torch.float64, device="cuda")
    assert lib().kmpc_observe_batch(0, len(c["rec"]), ptr(r2), ptr(dev(c["z"])), C.c_void_p(s8.data_ptr() + 48), 8, ptr(dev(c["params"])), 0.1, OR.L_A, OR.L_B,
                                    c["gate"], c["v_min"], c["psi_cap"], ptr(e2), None, None, None, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(r2.cpu().numpy(), got[0]) and np.array_equal(e2.cpu().numpy(), got[1], equal_nan=True)


# ---------------------------------------------------------------- 2: a 100-call recursion
def test_recursion_follows_the_restatement():
    """tests/observer_ref.py::recursion_case through vehicle_sim.DisturbanceObserver: 65 vehicles (one wave and one lane), 100 calls from fresh
    records, constant disturbances of both signs, five vehicles below v_min.  Flags and counters exact, the rest within TOL_RUN = 10 x
    MEASURED_RUN; and the filter finds the three offsets of the 60 vehicles that move: after 100 open-loop periods each is within four standard
    deviations of the filter's own covariance (180 samples; the restatement's worst is 2.2).
    Measured on the MI355X: record state 2.842e-14, P 2.001e-16 relative, est 2.842e-14, dist 1.582e-15, innov 1.331e-13; bounds 1.2e-12 (10 ulp of
    500 m), 2.1e-15, 1.2e-12, 1.6e-14, 1.4e-12; d-hat within 1.87, 1.60, 2.19 standard deviations."""
    import torch
    from mkz_mpc_path_follower_amd.vehicle_sim import DisturbanceObserver
    k = OR.recursion_case()
    K, B = k["z"].shape[0], k["z"].shape[1]
    ob = DisturbanceObserver(B)
    assert np.array_equal(ob.params.cpu().numpy(), k["params"])
    z, u = dev(k["z"]), dev(k["u"])
    out = dict(rec=torch.empty((K, B, 40), dtype=torch.float64, device="cuda"), est=torch.empty((K, B, 4), dtype=torch.float64, device="cuda"),
               dist=torch.empty((K, B, 3), dtype=torch.float64, device="cuda"), innov=torch.empty((K, B, 4), dtype=torch.float64, device="cuda"),
               flags=torch.empty((K, B), dtype=torch.int32, device="cuda"))
    for j in range(K):
        ob.update(z[j], u, out=out["est"][j])
        out["rec"][j].copy_(ob.record); out["dist"][j].copy_(ob.dist); out["innov"][j].copy_(ob.innov); out["flags"][j].copy_(ob.flags)
    torch.cuda.synchronize()
    got = {n: t.cpu().numpy() for n, t in out.items()}
    exp = OR.run_recursion(k["z"], k["u"], k["params"])
    assert np.array_equal(got["flags"], exp["flags"]) and np.array_equal(got["rec"][:, :, OR.COUNT:OR.SKIPPED + 1], exp["rec"][:, :, OR.COUNT:OR.SKIPPED + 1])
    assert (got["flags"][0] == OR.INIT).all() and not got["flags"][1:].any() and (got["rec"][-1, :, OR.COUNT] == K).all()
    err = errors(got["rec"], exp["rec"], got["est"], exp["est"], got["dist"], exp["dist"], got["innov"], exp["innov"])
    print("100-call recursion against numpy: record state %.3e, P %.3e (relative), est %.3e, dist %.3e, innov %.3e" % tuple(err))
    assert (err <= TOL_RUN).all() and TOL_RUN.max() <= 1e-9
    sd = np.sqrt(got["rec"][-1, :60][:, [7 + OR.TRI[(i, i)] for i in (4, 5, 6)]])
    d = np.abs(got["dist"][-1, :60] - k["d"][:60])
    print("d-hat against the truth after 100 calls, moving vehicles: within %s, %s standard deviations" % (np.round(d.max(0), 4), np.round((d / sd).max(0), 2)))
    assert (d <= 4.0 * sd).all()
    ob.reset()
    assert not ob.record.any().item() and not ob.flags.any().item() and not ob.dist.any().item()


# ---------------------------------------------------------------- 3: B = 1 and B = 0
def test_one_vehicle_and_none():
    c = OR.single_call_case()
    kw = dict(gate=c["gate"], v_min=c["v_min"], psi_cap=c["psi_cap"])
    whole = observe(c["rec"], c["z"], c["u"], c["params"], **kw)
    for b in (0, 45, 75, 299):
        alone = observe(c["rec"][b:b + 1], c["z"][b:b + 1], c["u"][b:b + 1], c["params"][b:b + 1], **kw)
        for w, a in zip(whole, alone):
            assert np.array_equal(w[b], a[0], equal_nan=True), b
    L = lib()
    assert L.kmpc_observe_batch(0, 0, None, None, None, 2, None, 0.1, OR.L_A, OR.L_B, 0.0, 1.0, 0.2, None, None, None, None, None) == 0
    assert L.kmpc_cmd_offset_batch(0, 0, None, None, 0.5, 0.1, None, None) == 0
    from mkz_mpc_path_follower_amd.vehicle_sim import DisturbanceObserver
    import torch
    ob = DisturbanceObserver(0)
    e = ob.update(torch.empty((0, 4), dtype=torch.float64, device="cuda"), torch.empty((0, 2), dtype=torch.float64, device="cuda"))
    assert tuple(e.shape) == (0, 4) and tuple(ob.offset(torch.empty((0, 2), dtype=torch.float64, device="cuda")).shape) == (0, 2)


# ---------------------------------------------------------------- 4: the reduction against kmpc_estimate_batch on the device
def test_reduction_is_the_estimator_kernel():
    """p0 = q_dist = 0: words 0 ... 3, the ten words of the 4 x 4 block, est_out, innov_out, flags and both counters are kmpc_estimate_batch's on the
    same inputs, as numbers, exactly -- on the estimator's seeded single call (gate 3, psi_cap 0.2) and over its 256-vehicle, 100-call recursion"""
    import torch
    L = lib()
    c = E.single_call_case()
    B = len(c["rec"])
    r16, z, u, p8 = dev(c["rec"]), dev(c["z"]), dev(c["u"]), dev(c["params"])
    e16, i16 = torch.empty((B, 4), dtype=torch.float64, device="cuda"), torch.empty((B, 4), dtype=torch.float64, device="cuda")
    f16 = torch.empty((B,), dtype=torch.int32, device="cuda")
    assert L.kmpc_estimate_batch(0, B, ptr(r16), ptr(z), ptr(u), 2, ptr(p8), 0.1, E.L_A, E.L_B, c["gate"], ptr(e16), ptr(i16), ptr(f16), None) == 0
    got = observe(OR.from_estimator(c["rec"]), c["z"], c["u"], OR.reduced_params(c["params"]), gate=c["gate"])
    torch.cuda.synchronize()
    assert as_numbers(OR.to_estimator(got[0]), r16.cpu().numpy()) and as_numbers(got[1], e16.cpu().numpy()) and as_numbers(got[3], i16.cpu().numpy())
    assert np.array_equal(got[4], f16.cpu().numpy()) and not got[2].any()
    assert not got[0][:, 7 + np.setdiff1d(np.arange(OR.NP), OR.BLOCK4)].any()
    from mkz_mpc_path_follower_amd.vehicle_sim import DisturbanceObserver, Estimator
    k = E.consistency_case()
    K, B = k["z"].shape[0], k["z"].shape[1]
    est, ob = Estimator(B, q=E.CONS_Q, r=E.CONS_R), DisturbanceObserver(B, q=E.CONS_Q, r=E.CONS_R, q_dist=0.0, p0=0.0)
    z, u = dev(k["z"]), dev(k["u"])
    same = []
    pick = torch.as_tensor(np.r_[0:4, 7 + np.array(OR.BLOCK4), OR.COUNT, OR.SKIPPED]).cuda()
    for j in range(K):
        a, b = est.update(z[j], u), ob.update(z[j], u)
        same.append(torch.equal(a, b) and torch.equal(est.record, ob.record[:, pick]) and torch.equal(est.innov, ob.innov) and torch.equal(est.flags, ob.flags))
    torch.cuda.synchronize()
    assert all(same) and (ob.record[:, OR.COUNT] == K).all().item() and not ob.dist.any().item()


# ---------------------------------------------------------------- 5: a poisoned vehicle costs itself alone
def test_a_poisoned_vehicle_costs_itself_alone():
    """a NaN record word, a NaN z, a NaN params word and a negative r, in one vehicle each: the other 296 vehicles' outputs keep their bits"""
    c = OR.single_call_case()
    kw = dict(gate=c["gate"], v_min=c["v_min"], psi_cap=c["psi_cap"])
    whole = observe(c["rec"], c["z"], c["u"], c["params"], **kw)
    rec, z, params = c["rec"].copy(), c["z"].copy(), c["params"].copy()
    rec[110, 20] = np.nan; z[257, 0] = np.nan; params[150, 5] = np.nan; params[200, 8] = -params[200, 8]
    got = observe(rec, z, c["u"], params, **kw)
    bad = [110, 257, 150, 200]
    keep = np.setdiff1d(np.arange(300), bad)
    for w, g in zip(whole, got):
        assert np.array_equal(w[keep], g[keep], equal_nan=True)
    exp = OR.observe(rec, z, c["u"], params, **kw)
    assert np.array_equal(got[4], exp[4])
    assert (got[4][[110, 150]] & OR.RESET).all() and not got[0][[110, 150]].any() and np.array_equal(got[1][[110, 150]], z[[110, 150]]) and not got[2][[110, 150]].any()
    assert got[4][257] == OR.SKIP[0] and np.isfinite(got[0][257]).all()                     # a NaN z is a dropout
    assert np.array_equal(got[0][200], whole[0][200])                                       # r enters squared: a negative r is its positive twin


# ---------------------------------------------------------------- 6: the command offset
def test_cmd_offset_is_exact():
    """against numpy, bit for bit: both caps binding and not binding, latched, fresh and non-finite vehicles untouched, caps of 0 leave cmd's bits"""
    import torch
    L = lib()
    c = OR.single_call_case()
    rec = OR.observe(c["rec"], c["z"], c["u"], c["params"], gate=c["gate"])[0]
    rec[30, 6] = np.nan; rec[31, 5] = np.inf; rec[32, 6] = -np.inf
    rng = np.random.default_rng(2)
    cmd = rng.uniform(-1, 1, (300, 2))
    cmd[3] = (-0.0, -0.0)
    latch = np.zeros(300, dtype=bool); latch[10:20] = True; latch[290:] = True
    untouched = np.r_[10:20, 290:300, 30, 31, 32, 60:70]
    for acc_cap, df_cap, lt in ((0.3, 0.02, latch), (0.5, 0.1, latch), (5.0, 1.0, None), (0.0, 0.0, None), (0.0, 0.02, latch)):
        d = dev(cmd)
        assert L.kmpc_cmd_offset_batch(0, 300, ptr(dev(rec)), None if lt is None else ptr(dev(lt, torch.bool)), acc_cap, df_cap, ptr(d), None) == 0
        torch.cuda.synchronize()
        got = d.cpu().numpy()
        assert np.array_equal(got.view(np.int64), OR.cmd_offset(rec, lt, acc_cap, df_cap, cmd).view(np.int64))
        if lt is not None:
            assert np.array_equal(got[untouched].view(np.int64), cmd[untouched].view(np.int64))
        if acc_cap == 0.0:
            assert np.array_equal(got[:, 0].view(np.int64), cmd[:, 0].view(np.int64))
        if df_cap == 0.0:
            assert np.array_equal(got[:, 1].view(np.int64), cmd[:, 1].view(np.int64))
    moved = np.setdiff1d(np.arange(300), untouched)
    d = dev(cmd)
    assert L.kmpc_cmd_offset_batch(0, 300, ptr(dev(rec)), ptr(dev(latch, torch.bool)), 0.3, 0.02, ptr(d), None) == 0
    torch.cuda.synchronize()
    assert (d.cpu().numpy()[moved] != cmd[moved]).all()


# ---------------------------------------------------------------- 7: the loops at the reduction
NV, STEPS7 = 12, 40


def _path1_loop(kind, **kw):
    from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop, ClosedLoopFrenet
    from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory
    from mkz_mpc_path_follower_amd.vehicle_sim import SensorModel, VehicleSimulator
    import latency_ref as LR
    arr, lat0, lon0 = S.path_arrays("path1_decimated.npz")
    grt = GPSRefTrajectory(arrays=arr, traj_horizon=8, traj_dt=0.2, lat0=lat0, lon0=lon0)
    X0, Y0, P0, _ = LR.starts(NV)
    sim = VehicleSimulator(NV, X0=X0, Y0=Y0, Psi0=P0)
    sim.state[:, 3] = LR.VT
    kw = dict(sensor=SensorModel(NV, sigma=(0.3, 0.3, 0.02, 0.1), seed=7), **kw)
    if kind == "frenet":
        return ClosedLoopFrenet(grt, sim, 8, LR.VT, **kw)
    return ClosedLoop(grt, sim, N=8, target_vel=LR.VT, **kw)


@pytest.mark.parametrize("kind", ["cartesian", "frenet"])
@pytest.mark.parametrize("estimator_input", ["actuator", "command"])
def test_loops_at_the_reduction_are_the_estimator_loops(kind, estimator_input):
    """observer= at p0 = q_dist = 0 and psi_cap = acc_cap = df_cap = 0 against estimator=: 12 vehicles on path1 behind a noisy sensor, 40 periods,
    states, commands, statuses, latches, measurements, estimates and scores bit for bit"""
    import torch
    from mkz_mpc_path_follower_amd.vehicle_sim import DisturbanceObserver, Estimator
    a = _path1_loop(kind, estimator=Estimator(NV), estimator_input=estimator_input)
    ob = DisturbanceObserver(NV, q_dist=0.0, p0=0.0, psi_cap=0.0, acc_cap=0.0, df_cap=0.0)
    b = _path1_loop(kind, observer=ob, estimator_input=estimator_input)
    ha, hb = a.run(STEPS7, history=True), b.run(STEPS7, history=True)
    torch.cuda.synchronize()
    for k in ("state", "cmd", "status", "latch", "est", "est_filt", "score"):
        assert torch.equal(ha[k], hb[k]), k
    assert (ha["status"] == 0).all().item() and not hb["dist"].any().item() and tuple(hb["dist"].shape) == (STEPS7, NV, 3)
    assert b.dist is ob.dist and torch.equal(b.est_filt, hb["est_filt"][-1]) and (ob.record[:, OR.COUNT] == STEPS7).all().item()
    assert not torch.equal(ha["est"], ha["est_filt"])


def test_loop_options_are_checked():
    from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop
    from mkz_mpc_path_follower_amd.vehicle_sim import DisturbanceObserver, Estimator, LatencyCompensator
    loop = _path1_loop("cartesian")
    assert loop.observer is None and loop.dist is None
    for kw in (dict(observer=DisturbanceObserver(NV), estimator=Estimator(NV)), dict(observer=DisturbanceObserver(NV), compensator=LatencyCompensator(NV)),
               dict(observer=DisturbanceObserver(NV + 1)), dict(observer=DisturbanceObserver(NV), estimator_input="history")):
        with pytest.raises(ValueError):
            ClosedLoop(loop.grt, loop.sim, N=8, target_vel=6.0, **kw)
    with pytest.raises(ValueError):
        DisturbanceObserver(NV).update(loop.sim.state[:, 0:4], loop.sim.cmd)          # z must be contiguous
    with pytest.raises(ValueError):
        DisturbanceObserver(NV).offset(loop.sim.state[:, 6:8])


# ---------------------------------------------------------------- 8: the loop against the CPU loop, and the quarter condition on the device
OFFSETS = (0.0, 0.3)
ROADS8 = (0, 4, 3)               # observer_ref.LOOP_ROADS: neutral, bank + offset, grade
CPU_STEPS = 120


def test_loop_matches_the_cpu_loop_and_is_offset_free(oracle):
    """six vehicles on path3 from 58 % of its length at 6 m/s: the neutral row, a_lat = 1.5 with df_offset = 0.03, and a_long = -0.5, each once on the
    path and once 0.3 m to its left, observer= with its defaults, 200 periods on the device.  The first 120 periods against observer_ref.cpu_loop
    (the oracle's waypoints and solver, the restated plant, observer and offset): positions, the other states and commands, and d-hat within
    TOL_LOOP = 10 x MEASURED_LOOP, capped at 1e-6.  Every solve Optimal.  And the quarter condition on the device: in the two bank + offset vehicles
    |mean e_ct| over periods 100 ... 200 is at most a quarter of the same vehicles' in the same loop without observer=.
    Measured on the MI355X: positions within 1.618e-12 m, other states and commands 3.110e-11, d-hat 1.452e-13 of the CPU loop (the neutral vehicles;
    the disturbed ones 2.9e-13, 8.7e-14, 1.1e-14); |mean e_ct| 0.0224 and 0.0233 m with the observer against 0.5996 and 0.5996 m without; the grade
    vehicles end at 6.994 and 6.976 m/s (6.650 without) with da-hat -0.4938 and -0.4937; d-hat of the bank + offset vehicles (0.0172, 0.0527, 0.004)."""
    import torch
    from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop
    from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory
    from mkz_mpc_path_follower_amd.vehicle_sim import DisturbanceObserver, VehicleSimulator, road_params
    runs, tr = OR.cpu_loops(oracle, ROADS8, OFFSETS, steps=CPU_STEPS, modes=("observer",))
    X0, Y0, P0, _ = RR.loop_start(OFFSETS)
    order = [(ri, oi) for ri in ROADS8 for oi in range(2)]
    rows = np.concatenate([RR.rows(1, **OR.LOOP_ROADS[ri]) for ri, _ in order])
    oi_ = [oi for _, oi in order]
    arr, lat0, lon0 = S.path_arrays(RR.PATH)
    grt = GPSRefTrajectory(arrays=arr, traj_horizon=8, traj_dt=0.2, lat0=lat0, lon0=lon0)
    hist = {}
    for with_observer in (True, False):
        sim = VehicleSimulator(6, X0=X0[oi_], Y0=Y0[oi_], Psi0=P0[oi_], road=torch.as_tensor(rows))
        sim.state[:, 3] = RR.VT
        loop = ClosedLoop(grt, sim, N=8, target_vel=RR.VT, observer=DisturbanceObserver(6) if with_observer else None)
        out = loop.run(OR.LOOP_STEPS, history=True)
        torch.cuda.synchronize()
        hist[with_observer] = {k: out[k].cpu().numpy() for k in ("state", "cmd", "status", "latch") + (("dist", "est_filt") if with_observer else ())}
    g = hist[True]
    assert (g["status"] == 0).all() and (hist[False]["status"] == 0).all() and not g["latch"].any() and np.isfinite(g["state"]).all() and np.isfinite(g["dist"]).all()
    worst, n = np.zeros(3), CPU_STEPS
    for b, (ri, oi) in enumerate(order):
        r = runs[(ri, OFFSETS[oi], "observer")]
        assert (r["status"] == 0).all()
        dp = np.hypot(g["state"][:n + 1, b, 0] - r["state"][:, 0], g["state"][:n + 1, b, 1] - r["state"][:, 1]).max()
        do = max(np.abs(g["state"][:n + 1, b, 2:] - r["state"][:, 2:]).max(), np.abs(g["cmd"][:n, b] - r["cmd"]).max())
        dd = np.abs(g["dist"][:n, b] - r["dist"]).max()
        print("vehicle %d (%s, %.1f m beside the path) against the CPU loop: max |dpos| %.3e m, other states and commands %.3e, d-hat %.3e; d-hat after 200 "
              "periods %s" % (b, OR.LOOP_NAMES[ri], OFFSETS[oi], dp, do, dd, np.round(g["dist"][-1, b], 4)))
        worst = np.maximum(worst, (dp, do, dd))
    print("worst: %s (bounds %s)" % (worst, TOL_LOOP))
    ect = {w: np.stack([S.cross_track(tr[:, 4:6], h["state"][:, b, 0], h["state"][:, b, 1])[0] for b in range(6)], 1) for w, h in hist.items()}
    m_with, m_without = (np.abs(ect[w][OR.TAIL:OR.LOOP_STEPS + 1].mean(0)) for w in (True, False))
    print("|mean e_ct| over periods 100 ... 200 [m]: with observer %s, without %s" % (np.round(m_with, 4), np.round(m_without, 4)))
    print("grade vehicles: v ends %s m/s with the observer, %s without; da-hat %s" % (np.round(g["state"][-1, 4:6, 3], 3),
                                                                                     np.round(hist[False]["state"][-1, 4:6, 3], 3), np.round(g["dist"][-1, 4:6, 2], 4)))
    assert (worst <= TOL_LOOP).all() and TOL_LOOP.max() <= 1e-6
    assert (m_with[2:4] <= 0.25 * m_without[2:4]).all()
    assert (np.abs(g["dist"][-1, 4:6, 2] + 0.5) <= 0.05).all()
