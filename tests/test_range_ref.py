"""CPU side of the range sensor and leader tracker (include/kmpc_range.h: kmpc_range_default, kmpc_range_rec_init, kmpc_range_follow_batch): the
header's constants against the Python names, the fourth export list, both host functions and every argument refusal (no GPU needed: every check
comes before the first device call), properties of the numpy restatement tests/range_ref.py, and follow_ref's three-vehicle CPU platoon with
the stage behind the search."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import follow_ref as FR
import range_ref as RG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1   # KMPC_ERR_ARG
DP = C.POINTER(C.c_double)


def _code(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_header_constants_and_export_lists():
    from mkz_mpc_path_follower_amd import _lib, ref_traj as RT
    code = _code("kmpc_range.h")
    const = {k: int(v) for k, v in re.findall(r"\b(KMPC_RANGE[A-Z0-9_]*)\s*=\s*(\d+)", code)}
    assert [const["KMPC_RANGE_" + f.upper()] for f in RT.RANGE_FIELDS] == list(range(11)) and const["KMPC_RANGE_WORDS"] == RT.RANGE_WORDS == 16
    assert [const["KMPC_RANGEREC_" + f.upper()] for f in RT.RANGE_REC_FIELDS] == list(range(16)) and const["KMPC_RANGEREC_WORDS"] == 16
    assert RT.RANGE_FIELDS == RG.FIELDS and RT.RANGE_REC_FIELDS == RG.REC_FIELDS
    declared = sorted(set(re.findall(r"\b(kmpc_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(_lib.RANGE_EXPORTS) == ["kmpc_range_default", "kmpc_range_follow_batch", "kmpc_range_rec_init"]
    L = _lib.load()
    for name in _lib.RANGE_EXPORTS:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None
        assert name not in _lib.EXPORTS and name not in _lib.EXT_EXPORTS and name not in _lib.LANE_EXPORTS
    assert len(_lib.EXPORTS) == 60 and len(_lib.EXT_EXPORTS) == 3 and len(_lib.LANE_EXPORTS) == 4 and L.kmpc_abi_version() == 8
    for other in ("kmpc.h", "kmpc_follow.h", "kmpc_lanes.h"):
        assert "kmpc_range" not in _code(other) and "KMPC_RANGE" not in _code(other), other


def test_host_functions_and_row_checks():
    from mkz_mpc_path_follower_amd import _lib, ref_traj as RT
    L = _lib.load()
    r = np.full((3, 16), 7.0)
    assert L.kmpc_range_default(r.ctypes.data_as(DP), 3) == 0
    assert r[0].tolist() == [120.0, 0.25, 0.12, 0.0, 0.0, 1.0, 5.0, 0.01, 0.25, 0.0625, 0.0144, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert np.array_equal(r, np.tile(RG.DEFAULT_ROW, (3, 1)))
    rec = np.full((3, 16), 7.0)
    assert L.kmpc_range_rec_init(rec.ctypes.data_as(DP), 3) == 0 and np.array_equal(rec, RG.fresh_rec(3))
    assert rec[0, 5] == -1.0 and rec[0].sum() == -1.0
    for fn in ("kmpc_range_default", "kmpc_range_rec_init"):
        f = getattr(L, fn)
        assert f(None, 1) == ARG and fn.encode() in L.kmpc_last_error(None)
        assert f(r.ctypes.data_as(DP), -1) == ARG and f(None, 0) == 0
    assert np.array_equal(RT.range_default(), RG.DEFAULT_ROW)
    assert np.array_equal(RT.range_neutral()[:11], RG.neutral_rows(1)[0, :11])
    for bad in (dict(range_max=0.0), dict(range_max=-np.inf), dict(range_max=np.nan), dict(sigma_r=-0.1), dict(sigma_r=np.inf), dict(sigma_v=-1.0),
                dict(bias_r=np.nan), dict(bias_r=np.inf), dict(p_drop=-0.1), dict(p_drop=1.1), dict(filter=0.5), dict(filter=2.0),
                dict(coast_max=1.5), dict(coast_max=-1.0), dict(coast_max=1001.0), dict(q_gap=-1e-9), dict(q_v=-1.0), dict(r_gap=0.0), dict(r_v=0.0),
                dict(r_v=np.nan)):
        with pytest.raises(ValueError):
            RT.check_range_rows(RG.rows(2, **bad))
    RT.check_range_rows(RG.rows(2, range_max=np.inf, sigma_r=0.0, sigma_v=0.0, bias_r=-3.0, p_drop=1.0, filter=0.0, coast_max=1000.0, q_gap=0.0, q_v=0.0))
    RT.check_range_rows(RG.neutral_rows(2))
    junk = RG.rows(2)
    junk[:, 11:16] = np.nan          # read by nobody
    RT.check_range_rows(junk)
    with pytest.raises(ValueError):
        RT.check_range_rows(np.zeros((2, 8)))


def test_argument_checks_answer_before_any_device_call():
    from mkz_mpc_path_follower_amd import _lib
    L = _lib.load()
    p = C.c_void_p(64)   # never dereferenced: every call below is refused on the host
    q = dict(B=2, dt=0.1, truth=p, leader=p, vt=p, ts=8, vk=p, ks=4, frows=p, rrows=p, seed=1, period=0, id_base=0, cap=p, out=p, rec=p, meas=p)

    def call(**kw):
        a = dict(q, **kw)
        return L.kmpc_range_follow_batch(0, a["B"], a["dt"], a["truth"], a["leader"], a["vt"], a["ts"], a["vk"], a["ks"], a["frows"], a["rrows"],
                                         a["seed"], a["period"], a["id_base"], a["cap"], a["out"], a["rec"], a["meas"], None)
    for bad in (dict(B=-1), dict(ts=0), dict(ks=0), dict(ks=-4), dict(dt=0.0), dict(dt=-0.1), dict(dt=np.nan), dict(dt=np.inf), dict(period=-1),
                dict(period=2 ** 61), dict(truth=None), dict(leader=None), dict(vt=None), dict(vk=None), dict(frows=None), dict(rrows=None),
                dict(cap=None), dict(out=None), dict(rec=None), dict(B=0, ts=0), dict(B=0, dt=0.0), dict(B=0, period=-1)):
        assert call(**bad) == ARG, bad
        assert b"kmpc_range_follow_batch" in L.kmpc_last_error(None)
    # B == 0 succeeds without a launch, whatever the pointers
    assert call(B=0, truth=None, leader=None, vt=None, vk=None, frows=None, rrows=None, cap=None, out=None, rec=None, meas=None,
                period=2 ** 61 - 1) == 0


# ---------------------------------------------------------------- the restatement's own properties
def _behind_follow(d, rrows, rec=None, period=0, seed=3):
    f = FR.follow(d["s"], d["v"], d["path_id"], d["present"], d["rows"], d["v_cap"])
    B = len(d["s"])
    o = RG.step(np.stack([f["gap"], f["v_lead"]], 1), f["leader"], d["v"], d["v"], d["rows"], rrows, seed, period, 0, d["v_cap"],
                RG.fresh_rec(B) if rec is None else rec, 0.1)
    return f, o


@pytest.mark.parametrize("B", (1, 65, 257, 1025))
def test_neutral_row_is_follow_bit_for_bit(B):
    """behind follow_ref.follow on follow_ref.draw (bad vehicles, absent ones, three paths), the neutral row gives follow()'s v_out with the same
    bits, call after call on one record, and the same bound decisions; whoever has a leader is tracked and nobody else"""
    rec = None
    for call in range(3):
        d = FR.draw(B, seed=call)
        f, o = _behind_follow(d, RG.neutral_rows(B), rec, period=call)
        rec = o["rec"]
        assert o["v_out"].tobytes() == f["v_out"].tobytes(), (B, call)
        assert np.array_equal(o["bound"], f["bound"]) and np.array_equal(o["track"], f["leader"] >= 0) and np.array_equal(o["det"], o["track"])
        has = f["leader"] >= 0
        assert rec[has, RG.GAP_HAT].tobytes() == f["gap"][has].tobytes() and (rec[has, RG.MAX_EGAP] == 0.0).all()
    assert (rec[:, RG.N] == 3.0).all() and (rec[:, RG.N_DROP] == 0).all() and (rec[:, RG.N_OUT] == 0).all()


def test_certain_dropout_coasts_then_hands_the_cap_through():
    """one follower 30 m behind a leader, detected once (P_DROP = 0), then P_DROP = 1: COAST_MAX = 4 periods of coasting on the prediction -- the
    cap stays the law's on the predicted gap -- then the track is given up and v_cap passes with its own bits.  A fresh record under P_DROP = 1
    never starts a track at all."""
    fr = FR.rows(1)
    cap = np.array([9.0])
    truth, lead, v = np.array([[30.0, 4.0]]), np.array([0]), np.array([6.0])
    o = RG.step(truth, lead, v, v, fr, RG.rows(1, coast_max=4.0), 1, 0, 0, cap, RG.fresh_rec(1), 0.1)
    assert o["det"][0] and o["new"][0] and o["bound"][0] and o["v_out"][0] < 9.0
    rr = RG.rows(1, coast_max=4.0, p_drop=1.0)
    rec = o["rec"]
    g = rec[0, RG.GAP_HAT]
    for k in range(1, 5):
        o = RG.step(truth, lead, v, v, fr, rr, 1, k, 0, cap, rec, 0.1)
        rec = o["rec"]
        g = g + 0.1 * (rec[0, RG.V_HAT] - 6.0)
        assert not o["det"][0] and o["drop"][0] and o["track"][0] and rec[0, RG.COAST] == k and o["meas"][0, 3] == k and np.isnan(o["meas"][0, 0])
        assert o["bound"][0] and o["v_out"][0] < 9.0 and abs(rec[0, RG.GAP_HAT] - g) < 1e-12
    o = RG.step(truth, lead, v, v, fr, rr, 1, 5, 0, cap, rec, 0.1)
    assert o["lost"][0] and not o["track"][0] and o["rec"][0, RG.TRACK_ID] == -1.0 and o["rec"][0, RG.N_LOST] == 1.0
    assert o["v_out"].tobytes() == cap.tobytes()
    assert o["rec"][0, RG.N_DROP] == 5.0 and o["rec"][0, RG.N_DETECT] == 1.0 and o["rec"][0, RG.N] == 6.0
    rec = RG.fresh_rec(1)
    for k in range(8):
        o = RG.step(truth, lead, v, v, fr, rr, 1, k, 0, cap, rec, 0.1)
        rec = o["rec"]
        assert not o["det"][0] and not o["track"][0] and o["v_out"].tobytes() == cap.tobytes()
    assert rec[0, RG.N_NEW] == 0.0 and rec[0, RG.N_LOST] == 0.0 and rec[0, RG.N_DROP] == 8.0


def test_a_leader_change_starts_a_new_track_in_the_same_period():
    fr, cap, v = FR.rows(1), np.array([9.0]), np.array([6.0])
    rr = RG.rows(1, sigma_r=0.0, sigma_v=0.0)
    o = RG.step(np.array([[40.0, 5.0]]), np.array([3]), v, v, fr, rr, 1, 0, 0, cap, RG.fresh_rec(1), 0.1)
    o = RG.step(np.array([[39.9, 5.0]]), np.array([3]), v, v, fr, rr, 1, 1, 0, cap, o["rec"], 0.1)
    assert o["rec"][0, RG.TRACK_ID] == 3.0 and o["rec"][0, RG.N_NEW] == 1.0 and o["rec"][0, RG.P00] < rr[0, 9]
    o = RG.step(np.array([[12.0, 2.0]]), np.array([7]), v, v, fr, rr, 1, 2, 0, cap, o["rec"], 0.1)     # somebody cut in
    rec = o["rec"]
    assert o["new"][0] and rec[0, RG.TRACK_ID] == 7.0 and rec[0, RG.N_NEW] == 2.0 and rec[0, RG.N_LOST] == 0.0
    assert rec[0, RG.GAP_HAT] == 12.0 and rec[0, RG.V_HAT] == 2.0 and rec[0, RG.P00:RG.P11 + 1].tolist() == [rr[0, 9], 0.0, rr[0, 10]]
    # the leader changes while nothing is detected (beyond the range limit): the old track is dropped, not coasted onto the new leader
    o = RG.step(np.array([[500.0, 2.0]]), np.array([8]), v, v, fr, rr, 1, 3, 0, cap, rec, 0.1)
    assert o["lost"][0] and o["out"][0] and not o["track"][0] and o["v_out"].tobytes() == cap.tobytes()
    # a follower that does not know its own speed detects nothing and loses its track at once
    o = RG.step(np.array([[12.0, 2.0]]), np.array([7]), v, np.array([np.nan]), fr, rr, 1, 3, 0, cap, rec, 0.1)
    assert not o["det"][0] and o["lost"][0] and o["v_out"].tobytes() == cap.tobytes()


def test_draws_do_not_depend_on_the_fleets_size_or_the_shard():
    d = RG.draw(257)
    whole = RG.run(d)
    lo, hi = RG.run(d, sl=slice(0, 100)), RG.run(d, id_base=100, sl=slice(100, 257))
    for c in range(3):
        for k in ("v_out", "rec", "meas"):
            a, b = whole[c][k], np.concatenate([lo[c][k], hi[c][k]])
            assert np.array_equal(np.isnan(a), np.isnan(b)) and a[~np.isnan(a)].tobytes() == b[~np.isnan(b)].tobytes(), (c, k)
    n0, n1, u = RG.draws(1000, 9, 4)
    m0, m1, w = RG.draws(10, 9, 4, id_base=990)
    assert np.array_equal(n0[990:], m0) and np.array_equal(n1[990:], m1) and np.array_equal(u[990:], w)
    # another period, another seed, another stage's tag: other numbers
    assert not np.array_equal(RG.draws(10, 9, 5)[0], n0[:10]) and not np.array_equal(RG.draws(10, 8, 4)[0], n0[:10])
    n = np.concatenate([n0, n1])
    assert abs(n.mean()) < 0.1 and abs(n.std() - 1.0) < 0.05 and 0.45 < u.mean() < 0.55 and (u > 0).all() and (u < 1).all()


def test_a_vehicle_with_nan_inputs_changes_only_its_own_outputs():
    d = RG.draw(65, calls=1)
    base = RG.run(d)[0]
    for key in ("truth", "v_true", "v_known", "range_rows", "follow_rows"):
        e = {k: ([a.copy() for a in v] if isinstance(v, list) else v.copy()) for k, v in d.items()}
        tgt = e[key][0] if isinstance(e[key], list) else e[key]
        tgt[17] = np.nan
        o = RG.run(e)[0]
        others = np.arange(65) != 17
        for k in ("v_out", "rec", "meas"):
            a, b = base[k][others], o[k][others]
            assert np.array_equal(np.isnan(a), np.isnan(b)) and a[~np.isnan(a)].tobytes() == b[~np.isnan(b)].tobytes(), (key, k)


def test_the_filter_beats_the_raw_measurement_at_constant_truth():
    """a follower and its leader both at 5 m/s, 25 m apart, 400 periods at SIGMA_R = 0.5 m (R_GAP = 0.25 to match): the variance of GAP_HAT over the
    last 300 periods is below that of z_r, and its mean is the truth to within the noise"""
    fr, cap, v = FR.rows(1), np.array([9.0]), np.array([5.0])
    rr = RG.rows(1, sigma_r=0.5, r_gap=0.25)
    rec, zs, gs = RG.fresh_rec(1), [], []
    for k in range(400):
        o = RG.step(np.array([[25.0, 5.0]]), np.array([0]), v, v, fr, rr, 42, k, 0, cap, rec, 0.1)
        rec = o["rec"]
        zs.append(o["meas"][0, 0]); gs.append(rec[0, RG.GAP_HAT])
    zs, gs = np.array(zs[100:]), np.array(gs[100:])
    print("variance of z_r %.4f m^2, of GAP_HAT %.4f m^2; means %.3f, %.3f m" % (zs.var(), gs.var(), zs.mean(), gs.mean()))
    assert 0.15 < zs.var() < 0.40 and gs.var() < 0.5 * zs.var() and abs(gs.mean() - 25.0) < 0.15
    assert rec[0, RG.N_DETECT] == 400.0 and rec[0, RG.N_NEW] == 1.0 and 0.0 < rec[0, RG.P00] < 0.25


def test_counts_are_consistent_on_the_draw():
    for B in (257, 1025):
        outs = RG.run(RG.draw(B))
        rec = outs[-1]["rec"]
        assert (rec[:, RG.N] == 3.0).all() and (rec[:, RG.N_DETECT] + rec[:, RG.N_DROP] + rec[:, RG.N_OUT] <= rec[:, RG.N]).all()
        assert (rec[:, RG.N_LOST] <= rec[:, RG.N_NEW]).all() and sum(o["lost"].sum() for o in outs) > 0 and sum(o["new"].sum() for o in outs[1:]) > 0
        for o in outs:
            assert np.array_equal(o["track"], o["rec"][:, RG.TRACK_ID] >= 0.0) and (o["v_out"][~o["bound"]] == RG.draw(B)["v_cap"][~o["bound"]]).all()


# ---------------------------------------------------------------- the CPU platoon
def test_neutral_radar_platoon_is_the_plain_platoon_bit_for_bit(oracle):
    r0, _, _ = FR.cached_platoon(oracle, "path1", True)
    r, _, _ = RG.cached_platoon(oracle, "path1", "neutral", RG.neutral_rows(3))
    for k in ("state", "cmd", "status", "v_follow", "gap", "leader", "stat"):
        assert np.array_equal(r[k], r0[k]), k
    assert np.array_equal(r["v_ideal"], r0["v_follow"]) and np.array_equal(r["gap_seen"][:, 1:], r0["gap"][:, 1:]) and np.isposinf(r["gap_seen"][:, 0]).all()


def test_noisy_radar_platoon_keeps_its_distance_on_the_cpu(oracle):
    """follow_ref.CASES["path1"] with SIGMA_R = 0.5 m, P_DROP = 0.2, FILTER = 1: no contact in any period and every solve Optimal"""
    r, _, _ = RG.cached_platoon(oracle, "path1", "noisy", RG.rows(3, sigma_r=0.5, p_drop=0.2, filter=1.0))
    rec = r["rec"]
    print("noisy radar platoon: smallest gaps %s m, detections %s, drops %s, rms gap error %s m, largest %s m"
          % (np.round(r["stat"][:, 4], 3), rec[:, RG.N_DETECT].astype(int).tolist(), rec[:, RG.N_DROP].astype(int).tolist(),
             np.round(np.sqrt(rec[:, RG.SUM_EGAP2] / 150.0), 3), np.round(rec[:, RG.MAX_EGAP], 3)))
    assert not r["stop"] and np.isfinite(r["state"]).all() and (r["status"] == 0).all()
    assert (r["stat"][:, 3] == 0).all() and (r["gap"] >= 0.0).all() and (r["final_gap"] >= 0.0).all()
    assert (rec[1:, RG.N_DROP] > 10).all() and (rec[1:, RG.N_DETECT] + rec[1:, RG.N_DROP] == 150).all() and rec[0, RG.N_DETECT] == 0


def test_the_draws_stay_clear_of_the_bound_decision():
    """tests/test_range.py excuses N_BOUND where the restated |v_f - v_cap| lies within the derived bound on v_cap_out (range_ref.bounds), and at
    most 1 % of a draw: the restatement's draws stay under that on every size and seed the device tests use (on continuous draws: nobody)"""
    for B in RG.SIZES:
        for seed in (0, 1):
            d = RG.draw(B, seed)
            outs = RG.run(d)
            for o, b in zip(outs, RG.bounds(d["follow_rows"], d["range_rows"], outs, RG.DT)):
                assert np.isfinite(b["v_out"]).all() and (b["v_out"] < 1e-10).all() and (b["gap_hat"] < 1e-10).all() and (b["v_hat"] < 1e-10).all()
                assert (o["margin"] <= b["v_out"]).sum() <= 0.01 * B, (B, seed)
