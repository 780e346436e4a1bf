"""CPU side of the state estimator (kmpc_estimate_batch): the numpy restatement of tests/estimator_ref.py against the textbook joint update, against
a finite difference of its own predict step and against the statistics a consistent filter must show; the inputs of the GPU tests; the argument checks
of the entry point (all before any device call) and the host-side validation of vehicle_sim.Estimator."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import estimator_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sequential_update_is_the_joint_update():
    """H = I, R diagonal: four scalar updates in a row are x + P (P + R)^-1 nu and P - P (P + R)^-1 P.  1e-12 relative to the largest entry of the
    joint result (the 4 x 4 systems here have condition numbers of a few hundred: rounding leaves 1e-14 ... 1e-13)."""
    rng = np.random.default_rng(3)
    B = 200
    P = E.random_spd(rng, B)
    xh = np.stack([rng.uniform(-500, 500, B), rng.uniform(-500, 500, B), rng.uniform(-2, 2, B), rng.uniform(0, 20, B)], 1)
    r2 = (np.array([0.2, 0.2, 0.02, 0.1]) * rng.uniform(0.5, 2.0, (B, 4))) ** 2
    nu = rng.normal(0, 1, (B, 4)) * np.sqrt(P[:, range(4), range(4)] + r2)
    z = xh + nu
    x1, P1 = xh.copy(), E.full_to_tri(P)
    for c in range(4):
        x1, P1, _, sk = E.update_channel(x1, P1, c, z[:, c], r2[:, c])
        assert not sk.any()
    G = P @ np.linalg.inv(P + r2[:, :, None] * np.eye(4))
    xj = xh + np.einsum("bij,bj->bi", G, z - xh)
    Pj = P - G @ P
    ex = np.abs(x1 - xj).max() / np.abs(xj).max()
    eP = (np.abs(E.tri_to_full(P1) - Pj).max((1, 2)) / np.abs(Pj).max((1, 2))).max()
    print("sequential against joint: x %.3e, P %.3e (relative)" % (ex, eP))
    assert ex < 1e-12 and eP < 1e-12


def test_jacobian_is_the_derivative_of_the_predict_step():
    """central difference, h = 1e-6, states of order 1..20: truncation h^2 f''' / 6 < 1e-11, rounding eps |f| / h < 2e-16 * 20 / 1e-6 = 4e-9 -> 1e-8"""
    rng = np.random.default_rng(4)
    B, h = 100, 1e-6
    xh = np.stack([rng.uniform(-1, 1, B), rng.uniform(-1, 1, B), rng.uniform(-3, 3, B), rng.uniform(1, 20, B)], 1)
    u = np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.5, 0.5, B)], 1)
    F = E.jacobian(xh, u, 0.1)
    fd = np.empty_like(F)
    for j in range(4):
        d = np.zeros(4); d[j] = h
        fd[:, :, j] = (E.model_step(xh + d, u, 0.1)[0] - E.model_step(xh - d, u, 0.1)[0]) / (2 * h)
    assert np.abs(F - fd).max() < 1e-8, np.abs(F - fd).max()
    # predict's P is F P F^T + Q with that F
    P = E.random_spd(rng, B)
    q2 = np.tile(np.array([0.02, 0.02, 0.01, 0.1]) ** 2, (B, 1))
    _, P1 = E.predict(xh, E.full_to_tri(P), u, q2, 0.1)
    want = F @ P @ F.transpose(0, 2, 1) + q2[:, :, None] * np.eye(4)
    assert np.abs(E.tri_to_full(P1) - want).max() < 1e-14


def test_single_call_case_has_the_groups_it_promises():
    c = E.single_call_case()
    rec, z = c["rec"], c["z"]
    assert rec.shape == (300, 16) and (rec[70:, 3] == 0).sum() >= 15 and np.abs(rec[:, 0:2]).max() > 400
    assert (np.linalg.eigvalsh(E.tri_to_full(rec[70:, 4:14])) > 0).all()
    out, est, innov, flags = E.estimate(rec, z, c["u"], c["params"], gate=c["gate"])
    assert (np.sign(rec[:20, 2]) != np.sign(z[:20, 2])).all() and (flags[:20] == 0).all() and np.abs(innov[:20, 2]).max() <= 2.0 + 1e-9
    assert np.abs(E.wrap(est[:20, 2] - rec[:20, 2])).max() < 0.5              # the estimate stayed at the cut instead of swinging round the circle
    for k in range(20):
        ch = k % 4
        assert flags[20 + k] == E.SKIP[ch] and out[20 + k, 15] == rec[20 + k, 15] + 1 and np.isfinite(out[20 + k]).all()
        assert flags[40 + k] & E.SKIP[ch] and out[40 + k, 15] >= rec[40 + k, 15] + 1
    ordinary = np.r_[0:20, 70:300]
    assert (flags[ordinary] == 0).all() and (out[ordinary, 14] == rec[ordinary, 14] + 1).all() and (out[ordinary, 15] == rec[ordinary, 15]).all()
    assert np.abs(innov[ordinary] - c["n"][ordinary]).max() < 1e-9           # whitening in the order x, y, psi, v is the Cholesky factorisation
    assert (flags[60:68] == E.INIT).all() and np.array_equal(est[60:68], z[60:68]) and (out[60:68, 14] == 1).all()
    assert np.array_equal(out[60:68, [4, 8, 11, 13]], c["params"][60:68, 4:8] ** 2) and not out[60:68][:, [5, 6, 7, 9, 10, 12, 15]].any()
    assert flags[68] == E.SKIP[1] and flags[69] == E.SKIP[3] and not out[68:70].any()
    assert np.isfinite(out).all() and (out[:, 3] >= 0).all() and (out[:, 2] >= -np.pi).all() and (out[:, 2] < np.pi).all()
    assert (out[rec[:, 3] == 0, 3] == np.maximum(0.0, out[rec[:, 3] == 0, 3])).all()


def test_containment_in_the_restatement():
    c = E.single_call_case()
    rec = c["rec"].copy()
    rec[5] = np.nan
    rec[6, 9] = np.inf
    params = c["params"].copy()
    params[7, 2] = np.nan
    out, est, innov, flags = E.estimate(rec, c["z"], c["u"], params, gate=c["gate"])
    for b in (5, 6, 7):
        assert flags[b] & E.RESET and not out[b].any() and np.array_equal(est[b], c["z"][b]) and not innov[b].any()
    ref = E.estimate(c["rec"], c["z"], c["u"], c["params"], gate=c["gate"])
    keep = np.r_[0:5, 8:300]
    for a, b in zip((out, est, innov, flags), ref):
        assert np.array_equal(a[keep], b[keep], equal_nan=a.dtype.kind == "f")     # est = z carries the NaN of the two fresh vehicles' measurements


def test_restatement_is_a_consistent_filter():
    """256 vehicles x 100 calls (99 updates, 25 344 innovations per channel), the committed seed.  A consistent filter's normalised innovations have
    unit variance: the mean of innov^2 has standard error sqrt(2 / 25344) = 0.009, the window is [0.9, 1.1].  Measured: 0.986, 1.004, 1.001, 1.004.
    rms error against the truth / the measurement's: 0.357, 0.354, 0.631, 0.785 (bounds: below 1 on every channel, below 0.5 on x and y)."""
    k = E.consistency_case()
    o = E.run_recursion(k["z"], k["u"], k["params"])
    assert (o["flags"][0] == E.INIT).all() and not o["flags"][1:].any() and np.array_equal(o["est"][0], k["z"][0])
    m = (o["innov"][1:] ** 2).mean((0, 1))
    d, dz = o["est"] - k["truth"], k["z"] - k["truth"]
    d[..., 2], dz[..., 2] = E.wrap(d[..., 2]), E.wrap(dz[..., 2])
    ratio = np.sqrt((d[1:] ** 2).mean((0, 1)) / (dz[1:] ** 2).mean((0, 1)))
    print("mean innov^2 %s over %d samples; rms error / measurement's %s" % (np.round(m, 4), o["innov"][1:, :, 0].size, np.round(ratio, 4)))
    assert o["innov"][1:, :, 0].size == 25344
    assert (m > 0.9).all() and (m < 1.1).all()
    assert (ratio < 1.0).all() and (ratio[0:2] < 0.5).all()
    assert (o["rec"][-1, :, 14] == 100).all() and not o["rec"][-1, :, 15].any()


def test_coasting_in_the_restatement():
    """NaN on x and y for 10 periods: P_xx and P_yy grow every period, the estimate stays finite, the skipped count rises by 20"""
    k = E.consistency_case()
    z = k["z"][:60, :16].copy()
    z[30:40, :, 0:2] = np.nan
    o = E.run_recursion(z, k["u"][:16], k["params"][:16])
    assert np.isfinite(o["est"]).all() and (o["flags"][30:40] == 3).all() and not o["flags"][40:].any()
    assert (np.diff(o["rec"][29:40, :, 4], axis=0) > 0).all() and (np.diff(o["rec"][29:40, :, 8], axis=0) > 0).all()
    assert (o["rec"][-1, :, 15] == 20).all()
    t = o["rec"][:, :, 4] + o["rec"][:, :, 8]       # trace of the position block: P_xx alone turns with the heading
    print("P_xx + P_yy before / at the end of / 20 periods after the dropout: %.5f %.5f %.5f" % (t[29].mean(), t[39].mean(), t[59].mean()))
    # re-converged: back near the value before (the steady state moves a little with v: measured ratio <= 1.07) and far below the coasting peak (>= 2.17 x)
    assert (t[59] < 1.25 * t[29]).all() and (t[59] < 0.6 * t[39]).all()


def test_fields_and_flags_match_the_header():
    from mkz_mpc_path_follower_amd import vehicle_sim as V
    hdr = open(os.path.join(ROOT, "include", "kmpc.h")).read()
    words = {n: int(v) for n, v in re.findall(r"KMPC_EST_([A-Z]+) = (\d+)", hdr)}
    assert words.pop("WORDS") == 16 and sorted(words.values()) == list(range(16))
    assert tuple(n.lower() for n, _ in sorted(words.items(), key=lambda kv: kv[1])) == V.ESTIMATOR_FIELDS == E.FIELDS
    par = {n: int(v) for n, v in re.findall(r"KMPC_ESTPAR_([A-Z_]+) = (\d+)", hdr)}
    assert par.pop("WORDS") == 8
    assert tuple(n.lower() for n, _ in sorted(par.items(), key=lambda kv: kv[1])) == V.ESTIMATOR_PARAM_FIELDS == E.PARAM_FIELDS
    fl = {n: int(v) for n, v in re.findall(r"KMPC_EST_FLAG_([A-Z_]+) = (\d+)", hdr)}
    assert fl == dict(SKIP_X=V.EST_SKIP_X, SKIP_Y=V.EST_SKIP_Y, SKIP_PSI=V.EST_SKIP_PSI, SKIP_V=V.EST_SKIP_V, INIT=V.EST_INIT, RESET=V.EST_RESET)
    assert (V.EST_SKIP_X, V.EST_SKIP_Y, V.EST_SKIP_PSI, V.EST_SKIP_V) == E.SKIP and (V.EST_INIT, V.EST_RESET) == (E.INIT, E.RESET)


def test_symbol_is_exported_and_the_abi_version_stays():
    from mkz_mpc_path_follower_amd import _lib
    L = _lib.load()
    assert "kmpc_estimate_batch" in _lib.EXPORTS and hasattr(L, "kmpc_estimate_batch") and L.kmpc_abi_version() == 8


def test_bad_arguments_are_refused_before_any_device_call():
    """every case answers KMPC_ERR_ARG without a GPU; the buffers are never read"""
    from mkz_mpc_path_follower_amd import _lib
    L = _lib.load()
    buf = C.cast(C.create_string_buffer(256), C.c_void_p)
    good = dict(B=2, rec=buf, z=buf, u=buf, stride=2, params=buf, dt=0.1, L_a=1.108, L_b=1.742, gate=0.0, est=buf)
    nan, inf = float("nan"), float("inf")
    for c in (dict(B=-1), dict(stride=1), dict(stride=0), dict(dt=0.0), dict(dt=-0.1), dict(dt=nan), dict(dt=inf), dict(L_a=0.0), dict(L_a=nan),
              dict(L_b=-1.0), dict(L_b=inf), dict(gate=-1.0), dict(gate=nan), dict(gate=inf),
              dict(rec=None), dict(z=None), dict(u=None), dict(params=None), dict(est=None)):
        a = dict(good, **c)
        rc = L.kmpc_estimate_batch(0, a["B"], a["rec"], a["z"], a["u"], a["stride"], a["params"], a["dt"], a["L_a"], a["L_b"], a["gate"], a["est"],
                                   None, None, None)
        assert rc == -1, c
        assert b"kmpc_estimate_batch" in L.kmpc_last_error(None)
    assert L.kmpc_estimate_batch(0, 0, None, None, None, 2, None, 0.1, 1.108, 1.742, 3.0, None, None, None, None) == 0      # B = 0: no launch
    assert L.kmpc_estimate_batch(0, 0, None, None, None, 1, None, 0.1, 1.108, 1.742, 3.0, None, None, None, None) == -1     # checked even then


def test_estimator_validation():
    from mkz_mpc_path_follower_amd.vehicle_sim import Estimator, SensorModel
    e = Estimator(3, device="cpu")
    assert tuple(e.params.shape) == (3, 8) and e.params[2].tolist() == [0.02, 0.02, 0.01, 0.1, 0.2, 0.2, 0.02, 0.1]
    assert tuple(e.record.shape) == (3, 16) and not e.record.any().item() and tuple(e.flags.shape) == (3,) and (e.dt, e.L_a, e.L_b, e.gate) == (0.1, 1.108, 1.742, 0.0)
    e = Estimator(3, q=0.0, r=[[0.1, 0.2, 0.3, 0.4]] * 3, gate=3.0, dt=0.05, device="cpu")      # q = 0 is a valid (over-confident) filter
    assert e.params[1].tolist() == [0.0, 0.0, 0.0, 0.0, 0.1, 0.2, 0.3, 0.4]
    for bad in (dict(q=-0.1), dict(q=float("nan")), dict(r=0.0), dict(r=(0.2, 0.2, 0.0, 0.1)), dict(r=float("inf")), dict(r=(1.0, 2.0)), dict(q=np.ones((2, 4))),
                dict(dt=0.0), dict(dt=float("nan")), dict(gate=-1.0), dict(gate=float("inf")), dict(L_a=0.0), dict(L_b=float("nan"))):
        with pytest.raises(ValueError):
            Estimator(3, device="cpu", **bad)
    s = SensorModel(3, sigma=[[0.5, 0.5, 0.0, 0.0], [0.1, 0.2, 0.02, 0.1], [0.0, 0.0, 0.0, 0.0]], device="cpu")
    e = Estimator.from_sensor(s, gate=3.0)
    assert e.B == 3 and e.gate == 3.0 and e.device == s.device
    assert e.params[:, 4:8].tolist() == [[0.5, 0.5, 1e-4, 1e-3], [0.1, 0.2, 0.02, 0.1], [1e-3, 1e-3, 1e-4, 1e-3]]
    assert e.params[0, 0:4].tolist() == [0.02, 0.02, 0.01, 0.1]
    for bad in (dict(r_floor=0.0), dict(r_floor=(1e-3, 1e-3)), dict(r_floor=float("nan")), dict(q=-1.0)):
        with pytest.raises(ValueError):
            Estimator.from_sensor(s, **bad)
