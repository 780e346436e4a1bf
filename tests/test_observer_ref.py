"""CPU side of the disturbance observer and the command offset (kmpc_observe_batch, kmpc_cmd_offset_batch): the numpy restatement of
tests/observer_ref.py against the estimator's restatement (the p0 = q_dist = 0 reduction, exact), against a central difference of its own step,
against the textbook joint update, its freeze rule and its containment; the argument checks of both entry points (all before any device call), the
host-side validation of vehicle_sim.DisturbanceObserver; and the one-vehicle CPU closed loop on a disturbed road with and without the stage.

The CPU loop (observer_ref.cpu_loop: road_ref.cpu_loop with the stage in it; path3 from 58 % of its length at 6 m/s, N = 8, the oracle's condensed
solver, 200 periods, the filters reading the truth).  Mean cross-track error over periods 100 ... 200 [m], recorded 2026-10-19:
    road row                      no filter   4-state filter (estimator_ref)   observer + offset
    neutral                        0.0078         0.0076                         0.0220   (rms 0.0118 / 0.0112 / 0.0420; corner max 0.621 / 0.980 / 0.879)
    a_lat = 1.5                    0.3204         0.5406                         0.0225   (d-hat: dpsi 0.0172, ddelta 0.0227)
    df_offset = 0.03               0.2771         0.4499                         0.0220   (ddelta-hat 0.0297)
    a_long = -0.5                  v ends 6.650   v ends 6.623                   v ends 6.994 m/s (da-hat -0.4938)
    a_lat = 1.5, df_offset = 0.03  0.5996         0.9950                         0.0224   (dpsi 0.0172, ddelta 0.0527)
Every solve Optimal.  The observer costs 0.014 m of mean and 0.03 m of rms on the clean road (tyre slip in the corner looks like a disturbance); the
neutral row and the 4-state column are recorded here and in DESIGN.md, not asserted.  DisturbanceObserver's defaults are the prototype's: the loop
gave no reason to move them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import estimator_ref as E
import observer_ref as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# central difference against the analytic Jacobian: measured 1.169e-09 (h = 1e-6, rounding eps |f| / h dominates); 10 x that
TOL_JACOBIAN = 1.2e-8
# sequential against joint update, relative to the largest entry of the joint result: the estimator's check's bound; measured x 1.1e-16, P 2.3e-15
TOL_JOINT = 1e-12


# ---------------------------------------------------------------- symbols and argument checks
def test_symbols_are_exported_and_the_abi_version_stays():
    from mkz_mpc_path_follower_amd import _lib
    L = _lib.load()
    for n in ("kmpc_observe_batch", "kmpc_cmd_offset_batch"):
        assert n in _lib.EXPORTS and hasattr(L, n)
    assert L.kmpc_abi_version() == 8


def test_fields_match_the_header():
    from mkz_mpc_path_follower_amd import vehicle_sim as V
    hdr = open(os.path.join(ROOT, "include", "kmpc.h")).read()
    words = {n: int(v) for n, v in re.findall(r"KMPC_OBS_([A-Z]+) = (\d+)", hdr)}
    assert words.pop("WORDS") == OR.WORDS == 40 and words.pop("COUNT") == OR.COUNT and words.pop("SKIPPED") == OR.SKIPPED and words.pop("P") == 7
    assert tuple(n.lower() for n, _ in sorted(words.items(), key=lambda kv: kv[1])) == V.OBSERVER_FIELDS and sorted(words.values()) == list(range(7))
    par = {n: int(v) for n, v in re.findall(r"KMPC_OBSPAR_([A-Z0-9_]+) = (\d+)", hdr)}
    assert par.pop("WORDS") == OR.PAR_WORDS == 16
    assert tuple(n.lower() for n, _ in sorted(par.items(), key=lambda kv: kv[1])) == V.OBSERVER_PARAM_FIELDS and sorted(par.values()) == list(range(14))
    assert len(OR.TRI) == OR.NP == 28 and OR.TRI[(6, 6)] == 27 and all(OR.TRI[(i, j)] == 7 * i - i * (i - 1) // 2 + (j - i) for (i, j) in OR.TRI)


def test_bad_arguments_are_refused_before_any_device_call():
    """every case answers KMPC_ERR_ARG without a GPU; the buffers are never read"""
    from mkz_mpc_path_follower_amd import _lib
    L = _lib.load()
    buf = C.cast(C.create_string_buffer(1024), C.c_void_p)
    good = dict(B=2, rec=buf, z=buf, u=buf, stride=2, params=buf, dt=0.1, L_a=1.108, L_b=1.742, gate=0.0, v_min=1.0, psi_cap=0.2, est=buf)
    nan, inf = float("nan"), float("inf")

    def observe(a):
        return L.kmpc_observe_batch(0, a["B"], a["rec"], a["z"], a["u"], a["stride"], a["params"], a["dt"], a["L_a"], a["L_b"], a["gate"], a["v_min"],
                                    a["psi_cap"], a["est"], None, None, None, None)
    for c in (dict(B=-1), dict(stride=1), dict(stride=0), dict(dt=0.0), dict(dt=-0.1), dict(dt=nan), dict(dt=inf), dict(L_a=0.0), dict(L_a=nan),
              dict(L_b=-1.0), dict(L_b=inf), dict(gate=-1.0), dict(gate=nan), dict(gate=inf),
              dict(v_min=-1.0), dict(v_min=nan), dict(v_min=inf), dict(psi_cap=-0.1), dict(psi_cap=nan), dict(psi_cap=inf),
              dict(rec=None), dict(z=None), dict(u=None), dict(params=None), dict(est=None)):
        assert observe(dict(good, **c)) == -1, c
        assert b"kmpc_observe_batch" in L.kmpc_last_error(None)
    empty = dict(good, B=0, rec=None, z=None, u=None, params=None, est=None)
    assert observe(empty) == 0                      # B = 0: no launch
    assert observe(dict(empty, stride=1)) == -1     # checked even then
    assert observe(dict(empty, v_min=0.0, psi_cap=0.0, gate=3.0)) == 0
    good = dict(B=2, rec=buf, latch=buf, acc_cap=0.5, df_cap=0.1, cmd=buf)

    def offset(a):
        return L.kmpc_cmd_offset_batch(0, a["B"], a["rec"], a["latch"], a["acc_cap"], a["df_cap"], a["cmd"], None)
    for c in (dict(B=-1), dict(acc_cap=-0.1), dict(acc_cap=nan), dict(acc_cap=inf), dict(df_cap=-0.1), dict(df_cap=nan), dict(df_cap=inf),
              dict(rec=None), dict(cmd=None)):
        assert offset(dict(good, **c)) == -1, c
        assert b"kmpc_cmd_offset_batch" in L.kmpc_last_error(None)
    assert offset(dict(good, B=0, rec=None, latch=None, cmd=None)) == 0
    assert offset(dict(good, B=0, rec=None, latch=None, cmd=None, acc_cap=nan)) == -1


def test_observer_validation():
    from mkz_mpc_path_follower_amd.vehicle_sim import DisturbanceObserver
    o = DisturbanceObserver(3, device="cpu")
    assert tuple(o.params.shape) == (3, 16) and o.params[2].tolist() == list(OR.Q + OR.Q_DIST + OR.R + OR.P0) + [0.0, 0.0]
    assert np.array_equal(o.params.numpy(), OR.param_rows(3))
    assert tuple(o.record.shape) == (3, 40) and not o.record.any().item() and tuple(o.dist.shape) == (3, 3) and tuple(o.flags.shape) == (3,)
    assert (o.dt, o.L_a, o.L_b, o.gate, o.v_min, o.psi_cap, o.acc_cap, o.df_cap) == (0.1, 1.108, 1.742, 0.0, OR.V_MIN, OR.PSI_CAP, OR.ACC_CAP, OR.DF_CAP)
    o = DisturbanceObserver(3, q_dist=0.0, p0=[[0.1, 0.2, 0.3]] * 3, psi_cap=0.0, acc_cap=0.0, df_cap=0.0, v_min=0.0, device="cpu")
    assert o.params[1, 4:7].tolist() == [0.0, 0.0, 0.0] and o.params[1, 11:14].tolist() == [0.1, 0.2, 0.3]
    for bad in (dict(q=-0.1), dict(q=float("nan")), dict(r=0.0), dict(r=float("inf")), dict(r=(1.0, 2.0)), dict(q_dist=-1e-3), dict(q_dist=(0.1, 0.1)),
                dict(q_dist=float("nan")), dict(p0=-0.1), dict(p0=float("inf")), dict(p0=np.ones((2, 3))), dict(dt=0.0), dict(gate=-1.0), dict(L_a=0.0),
                dict(v_min=-1.0), dict(psi_cap=float("nan")), dict(acc_cap=-0.5), dict(df_cap=float("inf"))):
        with pytest.raises(ValueError):
            DisturbanceObserver(3, device="cpu", **bad)


# ---------------------------------------------------------------- the restatement
def _as_numbers(a, b):
    """equal as numbers: a -0 may be a +0; NaN equals NaN (est = z carries the fresh vehicles' non-finite measurements)"""
    return np.array_equal(np.asarray(a) + 0.0, np.asarray(b) + 0.0, equal_nan=True)


def test_reduction_is_the_estimator_on_its_seeded_case():
    """p0 = q_dist = 0 and zero disturbances: the estimator's 16 words, est_out (at any psi_cap), innov_out and flags, as numbers, exactly"""
    c = E.single_call_case()
    want = E.estimate(c["rec"], c["z"], c["u"], c["params"], gate=c["gate"])
    for psi_cap, v_min in ((0.0, 0.0), (0.2, 1.0)):
        rec, est, dist, innov, flags = OR.observe(OR.from_estimator(c["rec"]), c["z"], c["u"], OR.reduced_params(c["params"]), gate=c["gate"],
                                                  v_min=v_min, psi_cap=psi_cap)
        assert _as_numbers(OR.to_estimator(rec), want[0]) and _as_numbers(est, want[1]) and _as_numbers(innov, want[2]) and np.array_equal(flags, want[3])
        assert not dist.any() and not rec[:, 4:7].any() and not rec[:, 37:40].any()
        rest = np.setdiff1d(np.arange(OR.NP), OR.BLOCK4)
        assert not rec[:, 7 + rest].any()


def test_reduction_is_the_estimator_over_its_recursion():
    """256 vehicles x 100 calls from fresh records: every call's record, estimate, innovations and flags"""
    k = E.consistency_case()
    want = E.run_recursion(k["z"], k["u"], k["params"])
    got = OR.run_recursion(k["z"], k["u"], OR.reduced_params(k["params"]))
    assert _as_numbers(OR.to_estimator(got["rec"]), want["rec"]) and _as_numbers(got["est"], want["est"])
    assert _as_numbers(got["innov"], want["innov"]) and np.array_equal(got["flags"], want["flags"]) and not got["dist"].any()


def test_jacobian_is_the_derivative_of_the_step():
    """central difference, h = 1e-6, of the restated step over all seven states, away from the wrap and the floor.  Truncation h^2 f''' / 6 < 1e-11,
    rounding eps |f| / h about 2e-16 x 20 / 1e-6 = 4e-9.  Measured 1.169e-09; the bound is 10 x that (TOL_JACOBIAN)."""
    rng = np.random.default_rng(4)
    B, h = 200, 1e-6
    xh = np.stack([rng.uniform(-1, 1, B), rng.uniform(-1, 1, B), rng.uniform(-3, 3, B), rng.uniform(1, 20, B), rng.uniform(-0.1, 0.1, B),
                   rng.uniform(-0.05, 0.05, B), rng.uniform(-0.5, 0.5, B)], 1)
    xh[:, 2] = np.clip(xh[:, 2], -2.9, 2.9)
    u = np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.5, 0.5, B)], 1)
    F = OR.jacobian(xh, u, 0.1)
    fd = np.empty_like(F)
    for j in range(OR.NS):
        d = np.zeros(OR.NS); d[j] = h
        fd[:, :, j] = (OR.model_step(xh + d, u, 0.1)[0] - OR.model_step(xh - d, u, 0.1)[0]) / (2 * h)
    err = np.abs(F - fd).max()
    print("analytic Jacobian against the central difference: %.3e (bound %.1e)" % (err, TOL_JACOBIAN))
    assert err <= TOL_JACOBIAN
    assert (np.abs(F[:, [0, 1, 2, 3], [5, 5, 5, 6]]) > 0).all()                         # the new columns are there
    # predict's P is F P F^T + Q with that F
    P = OR.random_spd(rng, B)
    q2 = np.tile(np.array(OR.Q + OR.Q_DIST) ** 2, (B, 1))
    _, P1 = OR.predict(xh, OR.full_to_tri(P), u, q2, 0.1, v_min=0.0)
    want = F @ P @ F.transpose(0, 2, 1) + q2[:, :, None] * np.eye(OR.NS)
    assert np.abs(OR.tri_to_full(P1) - want).max() < 1e-14


def test_sequential_update_is_the_joint_update():
    """H = [I 0], R diagonal: the four scalar updates over seven states are x + P H^T (H P H^T + R)^-1 nu and P - P H^T (...)^-1 H P.  Bound as the
    estimator's check: 1e-12 relative to the largest entry of the joint result; measured x 1.1e-16, P 2.3e-15."""
    rng = np.random.default_rng(3)
    B = 200
    P = OR.random_spd(rng, B)
    xh = np.concatenate([np.stack([rng.uniform(-500, 500, B), rng.uniform(-500, 500, B), rng.uniform(-2, 2, B), rng.uniform(0, 20, B)], 1),
                         rng.uniform(-0.1, 0.1, (B, 3))], 1)
    r2 = (np.array(OR.R) * rng.uniform(0.5, 2.0, (B, 4))) ** 2
    nu = rng.normal(0, 1, (B, 4)) * np.sqrt(P[:, range(4), range(4)] + r2)
    z = xh[:, 0:4] + nu
    x1, P1 = xh.copy(), OR.full_to_tri(P)
    for c in range(4):
        x1, P1, _, sk = OR.update_channel(x1, P1, c, z[:, c], r2[:, c])
        assert not sk.any()
    H = np.eye(4, OR.NS)
    G = P @ H.T @ np.linalg.inv(H @ P @ H.T + r2[:, :, None] * np.eye(4))
    xj = xh + np.einsum("bij,bj->bi", G, nu)
    Pj = P - G @ H @ P
    ex = np.abs(x1 - xj).max() / np.abs(xj).max()
    eP = (np.abs(OR.tri_to_full(P1) - Pj).max((1, 2)) / np.abs(Pj).max((1, 2))).max()
    print("sequential against joint: x %.3e, P %.3e (relative)" % (ex, eP))
    assert ex < TOL_JOINT and eP < TOL_JOINT


def test_freeze_rule():
    """v-hat before the step < v_min: q2 of dpsi and ddelta is not added, that of da and of the four states is; at a stop line P_dpsi and P_ddelta
    do not grow, however long the vehicle stands"""
    rng = np.random.default_rng(6)
    B = 8
    xh = np.zeros((B, OR.NS))
    xh[:, 3] = [0.0, 0.5, 0.999, 1.0, 1.001, 5.0, 0.0, 20.0]
    P = OR.full_to_tri(OR.random_spd(rng, B))
    u = np.zeros((B, 2))
    q2 = np.tile(np.array(OR.Q + OR.Q_DIST) ** 2, (B, 1))
    _, with_q = OR.predict(xh, P, u, q2, 0.1, v_min=1.0)
    _, no_q = OR.predict(xh, P, u, np.zeros((B, OR.NS)), 0.1, v_min=1.0)
    slow = xh[:, 3] < 1.0
    assert slow.tolist() == [True, True, True, False, False, False, True, False]
    for i in range(OR.NS):
        k = OR.TRI[(i, i)]
        frozen = slow & (i in (4, 5))
        assert np.array_equal(with_q[frozen, k], no_q[frozen, k]) and np.array_equal(with_q[~frozen, k], no_q[~frozen, k] + q2[~frozen, i])
    # 500 periods at rest, measurements arriving: the two frozen variances never rise, da's settles
    rec = np.zeros((1, OR.WORDS))
    z, par = np.array([[10.0, 20.0, 0.3, 0.0]]), OR.param_rows(1)
    p44, p55, p66 = [], [], []
    for _ in range(500):
        rec, _, _, _, _ = OR.observe(rec, z, np.zeros((1, 2)), par)
        p44.append(rec[0, 7 + OR.TRI[(4, 4)]]); p55.append(rec[0, 7 + OR.TRI[(5, 5)]]); p66.append(rec[0, 7 + OR.TRI[(6, 6)]])
    assert (np.diff(p44) <= 0).all() and (np.diff(p55) <= 0).all() and p44[-1] <= OR.P0[0] ** 2 and p55[-1] <= OR.P0[1] ** 2
    assert np.isfinite(rec).all() and p66[-1] < OR.P0[2] ** 2
    # the same vehicle with v_min = 0 (no freeze): the unobservable variances grow without bound
    rec = np.zeros((1, OR.WORDS))
    for _ in range(500):
        rec, _, _, _, _ = OR.observe(rec, z, np.zeros((1, 2)), par, v_min=0.0)
    assert rec[0, 7 + OR.TRI[(5, 5)]] > p55[-1] + 400 * OR.Q_DIST[1] ** 2


def test_single_call_case_has_the_groups_it_promises():
    c = OR.single_call_case()
    rec, z = c["rec"], c["z"]
    assert rec.shape == (300, 40) and (np.linalg.eigvalsh(OR.tri_to_full(rec[70:, 7:35])) > 0).all()
    assert (rec[70:100, 3] < c["v_min"]).all() and (rec[70:100, 3] == 0).sum() == 10 and (rec[100:, 3] > c["v_min"]).all()
    live = np.r_[0:60, 70:300]
    assert (rec[live, 4:7] > 0).any(0).all() and (rec[live, 4:7] < 0).any(0).all() and (np.abs(rec[live, 4]) > c["psi_cap"]).sum() > 30
    out, est, dist, innov, flags = OR.observe(rec, z, c["u"], c["params"], gate=c["gate"], v_min=c["v_min"], psi_cap=c["psi_cap"])
    assert (np.sign(rec[:20, 2]) != np.sign(z[:20, 2])).all() and (flags[:20] == 0).all()
    for k in range(20):
        ch = k % 4
        assert flags[20 + k] == OR.SKIP[ch] and out[20 + k, OR.SKIPPED] == rec[20 + k, OR.SKIPPED] + 1 and np.isfinite(out[20 + k]).all()
        assert flags[40 + k] & OR.SKIP[ch]
    ordinary = np.r_[0:20, 70:300]
    assert (flags[ordinary] == 0).all() and (out[ordinary, OR.COUNT] == rec[ordinary, OR.COUNT] + 1).all()
    assert (flags[60:68] == OR.INIT).all() and np.array_equal(est[60:68], z[60:68]) and (out[60:68, OR.COUNT] == 1).all() and not dist[60:68].any()
    d = [7 + OR.TRI[(i, i)] for i in range(7)]
    assert np.array_equal(out[60:68][:, d], np.concatenate([c["params"][60:68, 7:11], c["params"][60:68, 11:14]], 1) ** 2)
    assert flags[68] == OR.SKIP[1] and flags[69] == OR.SKIP[3] and not out[68:70].any()
    assert np.isfinite(out).all() and (out[:, 3] >= 0).all() and (out[:, 2] >= -np.pi).all() and (out[:, 2] < np.pi).all()
    assert np.array_equal(dist, out[:, 4:7]) and np.array_equal(est[:, [0, 1, 3]][live], out[live][:, [0, 1, 3]])
    capped = np.abs(out[live, 4]) > c["psi_cap"]
    assert capped.sum() > 30 and np.allclose(np.abs(OR.wrap(est[live, 2] - out[live, 2]))[capped], c["psi_cap"], atol=1e-12)


def test_containment_in_the_restatement():
    c = OR.single_call_case()
    kw = dict(gate=c["gate"], v_min=c["v_min"], psi_cap=c["psi_cap"])
    rec, params, z = c["rec"].copy(), c["params"].copy(), c["z"].copy()
    rec[5] = np.nan
    rec[6, 30] = np.inf
    rec[8, 5] = np.nan
    params[7, 5] = np.nan
    out, est, dist, innov, flags = OR.observe(rec, z, c["u"], params, **kw)
    for b in (5, 6, 7, 8):
        assert flags[b] & OR.RESET and not out[b].any() and np.array_equal(est[b], z[b]) and not innov[b].any() and not dist[b].any()
    ref = OR.observe(c["rec"], z, c["u"], c["params"], **kw)
    keep = np.r_[0:5, 9:300]
    for a, b in zip((out, est, dist, innov, flags), ref):
        assert np.array_equal(a[keep], b[keep], equal_nan=a.dtype.kind == "f")
    # the command offset leaves a latched, a fresh and a non-finite vehicle alone, and caps of 0 leave every bit
    cmd = np.random.default_rng(1).uniform(-1, 1, (300, 2))
    cmd[3, 0] = -0.0
    latch = np.zeros(300, dtype=bool); latch[10:20] = True
    r2 = ref[0].copy(); r2[30, 6] = np.nan; r2[31, 5] = np.inf
    got = OR.cmd_offset(r2, latch, 0.3, 0.02, cmd)
    same = np.r_[10:20, 30, 31, 60:70]
    assert np.array_equal(got[same], cmd[same]) and (got[np.setdiff1d(np.arange(300), same)] != cmd[np.setdiff1d(np.arange(300), same)]).all()
    step = np.abs(got - cmd)
    assert np.allclose(step.max(0), [0.3, 0.02], rtol=0, atol=1e-15) and ((step[:, 0] > 0) & (step[:, 0] < 0.29)).any() and ((step[:, 1] > 0) & (step[:, 1] < 0.019)).any()
    z0 = OR.cmd_offset(r2, None, 0.0, 0.0, cmd)
    assert np.array_equal(z0, cmd) and np.array_equal(np.signbit(z0), np.signbit(cmd))


# ---------------------------------------------------------------- the CPU closed loop
@pytest.mark.parametrize("ri", range(len(OR.LOOP_ROADS)), ids=[n.replace(" ", "") for n in OR.LOOP_NAMES])
def test_cpu_loop_is_offset_free(oracle, ri):
    """module docstring's table, one road row per case: every solve Optimal; ddelta-hat within 10 % of 0.03 in the offset row and da-hat within 10 %
    of -0.5 in the grade row at the end of the run (the model says they are exact at steady state); in each laterally disturbed row |mean e_ct| over
    periods 100 ... 200 at most a quarter of the same loop's without the observer (a quarter is the floor below which the stage is not doing its
    job; the ratios here are 0.04 ... 0.08)."""
    runs, _ = OR.cpu_loops(oracle, (ri,), modes=("none", "observer") if ri in OR.LATERAL else ("observer",))
    r = runs[(ri, 0.0, "observer")]
    tail = r["ect"][OR.TAIL:OR.LOOP_STEPS + 1]
    print("%s: observer mean e_ct %.4f m, rms %.4f m, max |e_ct| %.3f m, v ends %.3f m/s, d-hat %s" % (
        OR.LOOP_NAMES[ri], tail.mean(), np.sqrt((tail ** 2).mean()), np.abs(r["ect"]).max(), r["state"][-1, 3], np.round(r["dist"][-1], 4)))
    assert (r["status"] == 0).all() and np.isfinite(r["state"]).all() and np.isfinite(r["dist"]).all()
    road = OR.LOOP_ROADS[ri]
    if road == dict(df_offset=0.03):
        assert abs(r["dist"][-1, 1] - 0.03) <= 0.1 * 0.03
    if road == dict(a_long=-0.5):
        assert abs(r["dist"][-1, 2] + 0.5) <= 0.1 * 0.5
    if ri in OR.LATERAL:
        n = runs[(ri, 0.0, "none")]
        assert (n["status"] == 0).all()
        base = n["ect"][OR.TAIL:OR.LOOP_STEPS + 1].mean()
        print("%s: no observer mean e_ct %.4f m, ratio %.3f" % (OR.LOOP_NAMES[ri], base, abs(tail.mean()) / abs(base)))
        assert abs(tail.mean()) <= 0.25 * abs(base)
