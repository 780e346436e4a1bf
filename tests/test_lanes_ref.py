"""CPU side of the lane stage (include/kmpc_lanes.h: kmpc_lane_default, kmpc_lane_rec_init, kmpc_lane_step_fleet, kmpc_ref_offset_batch): the
header's constants against the Python names, the third export list, the host functions and every argument refusal (no GPU needed: every check
comes before the first device call), properties of the period on the numpy restatement tests/lanes_ref.py, and the overtaking scenario as a
three-vehicle CPU loop on two lanes and on one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import follow_ref as FR
import lanes_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1   # KMPC_ERR_ARG
DP = C.POINTER(C.c_double)


def test_header_constants_and_export_lists():
    from mkz_mpc_path_follower_amd import _lib, ref_traj as RT
    txt = open(os.path.join(ROOT, "include", "kmpc_lanes.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    const = {k: int(v) for k, v in re.findall(r"\b(KMPC_LANE[A-Z_0-9]*)\s*=\s*(\d+)", code)}
    assert [const["KMPC_LANE_" + f.upper()] for f in RT.LANE_FIELDS] == list(range(7)) and const["KMPC_LANE_WORDS"] == RT.LANE_WORDS == 8
    assert [const["KMPC_LANEREC_" + f.upper()] for f in RT.LANE_REC_FIELDS] == list(range(13)) and const["KMPC_LANEREC_WORDS"] == RT.LANE_REC_WORDS == 16
    assert RT.LANE_FIELDS == LR.FIELDS and RT.LANE_REC_FIELDS == LR.REC_FIELDS
    # words 4 ... 9 of the record are the follower's record, in its order
    assert RT.LANE_REC_FIELDS[4:10] == RT.FOLLOW_STAT_FIELDS
    declared = sorted(set(re.findall(r"\b(kmpc_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(_lib.LANE_EXPORTS) == ["kmpc_lane_default", "kmpc_lane_rec_init", "kmpc_lane_step_fleet", "kmpc_ref_offset_batch"]
    L = _lib.load()
    for name in _lib.LANE_EXPORTS:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None and name not in _lib.EXPORTS and name not in _lib.EXT_EXPORTS
    assert len(_lib.EXPORTS) == 60 and _lib.EXT_EXPORTS == ["kmpc_follow_default", "kmpc_follow_stat_init", "kmpc_follow_fleet"]
    assert L.kmpc_abi_version() == 8
    for other in ("kmpc.h", "kmpc_follow.h"):
        h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", other)).read(), flags=re.S)
        assert "kmpc_lane_" not in h and "kmpc_ref_offset" not in h


def test_host_functions():
    from mkz_mpc_path_follower_amd import _lib, ref_traj as RT
    L = _lib.load()
    r = np.full((3, 8), 7.0)
    assert L.kmpc_lane_default(r.ctypes.data_as(DP), 3) == 0
    assert r[0].tolist() == [1.0, 3.5, 1.0, 0.5, 20.0, 0.5, 1.0, 0.0] and np.array_equal(r, np.tile(LR.DEFAULT_ROW, (3, 1)))
    rec = np.full((3, 16), 7.0)
    assert L.kmpc_lane_rec_init(rec.ctypes.data_as(DP), 3) == 0 and np.array_equal(rec, LR.fresh_rec(3))
    assert rec[0, LR.MIN_GAP] == np.inf and rec[0, LR.LANE] == rec[0, LR.LANE_FROM] == rec[0, LR.OFFSET] == 0.0
    for fn in ("kmpc_lane_default", "kmpc_lane_rec_init"):
        f = getattr(L, fn)
        assert f(None, 1) == ARG and fn.encode() in L.kmpc_last_error(None)
        assert f(r.ctypes.data_as(DP), -1) == ARG and f(None, 0) == 0
    assert np.array_equal(RT.lane_default(), LR.DEFAULT_ROW)
    for bad in (dict(n_lanes=0), dict(n_lanes=33), dict(n_lanes=1.5), dict(n_lanes=np.nan), dict(width=0.0), dict(width=np.inf), dict(v_lat=0.0),
                dict(v_lat=np.nan), dict(gain=-0.1), dict(hold=-1), dict(hold=2.5), dict(clear_tol=-0.1), dict(clear_tol=np.nan),
                dict(keep_right=2), dict(keep_right=0.5)):
        with pytest.raises(ValueError, match="lane rows"):
            RT.check_lane_rows(LR.rows(2, **bad))
    RT.check_lane_rows(LR.rows(2, n_lanes=32, gain=0.0, hold=0, clear_tol=0.0, keep_right=0))
    junk = LR.rows(2)
    junk[:, 7] = np.nan           # read by nobody
    RT.check_lane_rows(junk)
    with pytest.raises(ValueError):
        RT.check_lane_rows(np.zeros((2, 7)))


def test_argument_checks_answer_before_any_device_call():
    from mkz_mpc_path_follower_amd import _lib
    L = _lib.load()
    p, p2 = C.c_void_p(64), C.c_void_p(128)   # never dereferenced: every call below is refused on the host
    q = dict(B=2, k=0, dt=0.1, s=p, ss=4, e=p, es=4, v=p, vs=8, pid=p, present=p, fr=p, lr=p, cap=p, out=p, occ_in=p, occ_out=p2, rec=p, gap=p,
             leader=p, nbr=p)

    def call(**kw):
        a = dict(q, **kw)
        return L.kmpc_lane_step_fleet(0, a["B"], a["k"], a["dt"], a["s"], a["ss"], a["e"], a["es"], a["v"], a["vs"], a["pid"], a["present"], a["fr"],
                                      a["lr"], a["cap"], a["out"], a["occ_in"], a["occ_out"], a["rec"], a["gap"], a["leader"], a["nbr"], None)
    for bad in (dict(B=-1), dict(k=-1), dict(ss=0), dict(es=0), dict(es=-4), dict(vs=0), dict(dt=0.0), dict(dt=-0.1), dict(dt=np.nan), dict(dt=np.inf),
                dict(s=None), dict(e=None), dict(v=None), dict(fr=None), dict(lr=None), dict(cap=None), dict(out=None), dict(occ_in=None),
                dict(occ_out=None), dict(rec=None), dict(occ_out=p), dict(B=0, ss=0), dict(B=0, dt=0.0)):
        assert call(**bad) == ARG, bad
        assert b"kmpc_lane_step_fleet" in L.kmpc_last_error(None)
    assert call(occ_out=p) == ARG and b"occ_in == occ_out" in L.kmpc_last_error(None)
    # B == 0 succeeds without a launch, whatever the pointers
    none = {k: None for k in ("s", "e", "v", "pid", "present", "fr", "lr", "cap", "out", "occ_in", "occ_out", "rec", "gap", "leader", "nbr")}
    assert call(B=0, **none) == 0

    def shift(B=2, H1=9, ref=p, off=p, stride=16):
        return L.kmpc_ref_offset_batch(0, B, H1, ref, off, stride, None)
    for bad in (dict(B=-1), dict(H1=0), dict(H1=-3), dict(stride=0), dict(ref=None), dict(off=None), dict(B=2 ** 30, H1=2), dict(B=0, H1=0)):
        assert shift(**bad) == ARG, bad
        assert b"kmpc_ref_offset_batch" in L.kmpc_last_error(None)
    assert shift(B=0, ref=None, off=None) == 0


# ---------------------------------------------------------------- the restatement's own properties
def _road(s, v, lanes, n_lanes=3, frm=None, k=0, e_ct=None, hold_left=0.0, offset=None, follow=None, **lane_kw):
    """vehicles at arclengths s, speeds v in `lanes` (leaving `frm`) on one path, every cap 30 m/s -> (step()'s dict, the inputs)"""
    s, v, lanes = np.asarray(s, dtype=np.float64), np.asarray(v, dtype=np.float64), np.asarray(lanes, dtype=np.float64)
    B = len(s)
    lr = LR.rows(B, n_lanes=n_lanes, **lane_kw)
    rec = LR.fresh_rec(B, lanes, lr[:, 1])
    if frm is not None:
        rec[:, LR.LANE_FROM] = frm
    if offset is not None:
        rec[:, LR.OFFSET] = offset
    rec[:, LR.HOLD_LEFT] = hold_left
    occ = LR.bit(rec[:, LR.LANE]) | LR.bit(rec[:, LR.LANE_FROM])
    e = rec[:, LR.OFFSET].copy() if e_ct is None else np.asarray(e_ct, dtype=np.float64)
    fr = FR.rows(B, **(follow or {}))
    return LR.step(s, e, v, None, None, fr, lr, np.full(B, 30.0), occ, rec, k, 0.1), dict(rec=rec, occ=occ, lr=lr, fr=fr)


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()


@pytest.mark.parametrize("B", [65, 257])
def test_one_lane_is_the_follower_bit_for_bit(B):
    """N_LANES = 1, everybody in lane 0 with fresh occupancy, on follow_ref.draw (bad vehicles included), three calls on one record: everything
    follow_ref.follow returns is the stage's, bit for bit; nobody changes lane, every offset stays 0 and the occupancy stays 1"""
    rec, stat, occ = LR.fresh_rec(B), None, np.ones(B, dtype=np.uint32)
    for k in range(3):
        d = FR.draw(B, seed=k, paths=3)
        e = FR.follow(d["s"], d["v"], d["path_id"], d["present"], d["rows"], d["v_cap"], stat)
        g = LR.step(d["s"], np.zeros(B), d["v"], d["path_id"], d["present"], d["rows"], LR.rows(B), d["v_cap"], occ, rec, k, 0.1)
        for key in ("v_out", "gap", "v_lead"):
            assert _bits(g[key], e[key]), (k, key)
        for key in ("leader", "bound", "safe_arm"):
            assert np.array_equal(g[key], e[key]), (k, key)
        assert _bits(g["rec"][:, 4:10], e["stat"][:, 0:6])
        assert (g["rec"][:, [0, 1, 2, 3, 10]] == 0.0).all() and (g["occ"] == 1).all() and (g["winners"][:, 1:] == -1).all()
        rec, stat, occ = g["rec"], e["stat"], g["occ"]


def test_a_vehicle_in_mid_change_leads_in_both_of_its_lanes():
    """vehicle 0, 30 m ahead, is moving from lane 0 to lane 1: it is the own-ahead winner of vehicle 1 in lane 0 and of vehicle 2 in lane 1, and the
    left-ahead winner of vehicle 1 as well; vehicle 3 in lane 2 has nobody in its own lane.  Vehicles 1, 2, 3 are one metre apart, so each is
    the other's neighbour behind or ahead"""
    o, _ = _road([100.0, 70.0, 69.0, 68.0], [3.0, 6.0, 6.0, 6.0], [1, 0, 1, 2], frm=[0, 0, 1, 2], offset=[1.0, 0.0, 3.5, 7.0])
    assert o["winners"][0].tolist() == [-1, -1, 3, -1, 1]          # nobody ahead; left of lane 1 vehicle 3 behind, right of it vehicle 1 behind
    assert o["winners"][1].tolist() == [0, 0, 2, -1, -1]           # lane 0: vehicle 0 in the own band AND in the left band
    assert o["winners"][2].tolist() == [0, -1, 3, 1, -1]           # lane 1: vehicle 0 in the own band; lane 0's nearest ahead is vehicle 1
    assert o["winners"][3].tolist() == [-1, -1, -1, 2, -1]         # lane 2: alone; no lane 3
    assert o["leader"].tolist() == [-1, 0, 0, -1] and o["occ"].tolist() == [3, 1, 2, 4]
    assert o["gap"][1] == 30.0 - 4.9 and o["gap"][2] == 31.0 - 4.9 and o["nbr"][3, 2].tolist() == [1.0 - 4.9, 6.0]
    assert o["nbr"][3, 0].tolist() == [np.inf, 0.0] and o["moved"].tolist() == [0, 0, 0, 0]


def test_lanes_zero_and_two_never_enter_lane_one_in_one_period():
    """a slow vehicle ahead in lane 0 (vehicle 1 behind it wants to move left) and a free lane 1 beside vehicle 2 in lane 2 (which wants to keep
    right), both alongside each other: in an even period only the left move happens, in an odd one only the right move -- and the period after,
    the other sees the first one's double occupancy right beside it and stays"""
    s, v, lanes = [60.0, 40.0, 40.0], [3.0, 6.0, 6.0], [0, 0, 2]
    for k0 in (0, 1):
        o, w = _road(s, v, lanes, k=k0, hold=0)
        assert o["moved"].tolist() == ([0, 1, 0] if k0 == 0 else [0, 0, -1])
        mover, other = (1, 2) if k0 == 0 else (2, 1)
        assert o["occ"][mover] == (0b011 if k0 == 0 else 0b110) and o["rec"][mover, LR.LANE] == 1.0
        e2 = o["rec"][:, LR.OFFSET].copy()
        o2 = LR.step(np.asarray(s), e2, np.asarray(v), None, None, w["fr"], w["lr"], np.full(3, 30.0), o["occ"], o["rec"], k0 + 1, 0.1)
        assert o2["moved"].tolist() == [0, 0, 0]                    # alongside, 0 m apart: the rear / front gap is below D_MIN
        assert o2["rec"][other, LR.LANE] == lanes[other] and o2["rec"][other, LR.N_CHANGES] == 0.0
    # without the parity rule's other half: in an even period the right mover alone stays, in an odd one the left mover alone
    assert _road([40.0], [6.0], [2], k=0)[0]["moved"].tolist() == [0] and _road([40.0], [6.0], [2], k=1)[0]["moved"].tolist() == [-1]


def test_ramp_lands_exactly_and_only_then_the_old_lane_is_released():
    """a vehicle moving from lane 0 to lane 1 (width 3.3: 3.3 is no sum of steps of 0.1): the offset climbs by V_LAT * dt per period, lands on
    LANE * WIDTH's own bits, the occupancy stays double until then AND until the vehicle itself is within CLEAR_TOL of the offset; then one bit"""
    lr, fr = LR.rows(1, n_lanes=2, width=3.3, hold=50), FR.rows(1)
    rec = LR.fresh_rec(1)
    rec[0, LR.LANE], rec[0, LR.HOLD_LEFT] = 1.0, 50.0
    occ, offs = np.array([3], dtype=np.uint32), []
    for k in range(40):
        at_target = rec[0, LR.OFFSET] == 1.0 * 3.3
        e_ct = rec[0, LR.OFFSET] - (0.6 if k < 36 else 0.4)        # the vehicle lags the commanded offset by 0.6 m, later by 0.4 m (CLEAR_TOL 0.5)
        o = LR.step(np.array([10.0]), np.array([e_ct]), np.array([5.0]), None, None, fr, lr, np.array([9.0]), occ, rec, k, 0.1)
        released = o["rec"][0, LR.LANE_FROM] == 1.0
        assert released == (at_target and k >= 36), k
        assert o["occ"][0] == (2 if released else 3)
        rec, occ = o["rec"], o["occ"]
        offs.append(rec[0, LR.OFFSET])
    assert offs[32] == 3.3 and offs[31] < 3.3 and offs[-1] == 3.3 and np.array_equal(offs[:5], np.cumsum(np.full(5, 0.1)))
    assert abs(offs[31] - 3.2) < 1e-12 and offs[31] != 3.2          # the ramp's sums do not hit 3.2's bits: the landing is by select
    assert rec[0, LR.MAX_ELANE] == pytest.approx(0.6) and rec[0, LR.N_CHANGES] == 0.0


def test_no_decision_while_hold_left_is_positive():
    """the left move of the parity test happens with HOLD_LEFT == 0 and not with HOLD_LEFT > 0, which counts down by one per period instead; a
    move sets HOLD_LEFT = HOLD"""
    s, v, lanes = [60.0, 40.0], [3.0, 6.0], [0, 0]
    o, w = _road(s, v, lanes, hold_left=[0.0, 2.0], hold=7)
    assert o["moved"].tolist() == [0, 0] and o["rec"][1, LR.HOLD_LEFT] == 1.0 and o["bound"][1]
    o1 = LR.step(np.asarray(s), np.zeros(2), np.asarray(v), None, None, w["fr"], w["lr"], np.full(2, 30.0), o["occ"], o["rec"], 2, 0.1)
    assert o1["moved"].tolist() == [0, 0] and o1["rec"][1, LR.HOLD_LEFT] == 0.0
    o2 = LR.step(np.asarray(s), np.zeros(2), np.asarray(v), None, None, w["fr"], w["lr"], np.full(2, 30.0), o1["occ"], o1["rec"], 4, 0.1)
    assert o2["moved"].tolist() == [0, 1] and o2["rec"][1, LR.HOLD_LEFT] == 7.0 and o2["rec"][1, LR.N_CHANGES] == 1.0
    # one lane: never a decision, whatever the hold
    assert _road(s, v, lanes, n_lanes=1)[0]["moved"].tolist() == [0, 0]
    # an unsafe rear: a faster vehicle close behind in the left lane keeps the follower where it is
    assert _road([60.0, 40.0, 30.0], [3.0, 6.0, 9.0], [0, 0, 1])[0]["moved"].tolist() == [0, 0, 0]


def test_relabelling_the_vehicles_relabels_the_outputs():
    """257 vehicles of the lane draw at DISTINCT arclengths (no ties): under a random permutation of the labels every vehicle keeps its own outputs'
    bits and record, and its five winners are the same vehicles under their new labels"""
    B = 257
    d = LR.draw(B, seed=5, paths=3, bad=False)
    rng = np.random.default_rng(4)
    d["s"] = 3.25 * rng.permutation(4 * B).astype(np.float64)[:B]
    a = LR.step_draw(d, 0)
    perm = rng.permutation(B)
    inv = np.argsort(perm)
    dp = {k: (v[perm] if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    b = LR.step_draw(dp, 0)
    assert (a["moved"] != 0).sum() >= 3 and (a["winners"] >= 0).sum(0).min() >= 20
    for k in ("v_out", "gap", "v_lead", "nbr", "rec"):
        assert _bits(b[k], a[k][perm]), k
    assert np.array_equal(b["occ"], a["occ"][perm]) and np.array_equal(b["moved"], a["moved"][perm])
    old = a["winners"][perm]
    assert np.array_equal(b["winners"], np.where(old >= 0, inv[np.maximum(old, 0)], -1))


def test_draws_cover_the_period():
    """the shared draw has what the parity test on the device needs: every search with winners, moves in both directions, releases, vehicles that
    are not usable, Gipps-arm caps"""
    seq = LR.calls(1025, 3)
    moved = np.stack([e["moved"] for _, e in seq])
    assert (moved[0] == 1).sum() > 10 and (moved[1] == -1).sum() > 5 and (moved[0] == -1).sum() == 0 and (moved[1] == 1).sum() == 0
    rel = sum(int(((d["rec"][:, 0] != d["rec"][:, 1]) & (e["rec"][:, 0] == e["rec"][:, 1])).sum()) for d, e in seq)
    assert rel > 5 and all((e["winners"] >= 0).sum(0).min() > 50 for _, e in seq) and sum(int(e["safe_arm"].sum()) for _, e in seq) > 50
    d, e = seq[0]
    bad = ~FR.usable(d["s"], d["v"], d["path_id"], d["present"])
    assert bad.sum() > 50 and _bits(e["rec"][bad][:, [0, 1, 2, 3]], d["rec"][bad][:, [0, 1, 2, 3]]) and (e["occ"][bad] == d["occ"][bad]).all()
    assert (e["rec"][:, LR.N] == 1.0).all() and (e["leader"][bad] == -1).all() and _bits(e["v_out"][bad], d["v_cap"][bad])


def test_ref_offset_restatement():
    ref = np.zeros((3, 9, 3))
    ref[:, :, 0], ref[:, :, 2] = np.arange(9.0), np.array([0.0, np.pi / 2, 0.3])[:, None]
    out = LR.ref_offset(ref, np.array([2.0, 2.0, 0.0]))
    assert np.allclose(out[0, :, 1], 2.0) and np.array_equal(out[0, :, 0], ref[0, :, 0])          # heading +x: left is +y
    assert np.allclose(out[1, :, 0], ref[1, :, 0] - 2.0) and np.allclose(out[1, :, 1], 0.0)     # heading +y: left is -x
    assert out[2].tobytes() == ref[2].tobytes() and np.array_equal(out[:, :, 2], ref[:, :, 2])


# ---------------------------------------------------------------- the overtaking scenario on the CPU
def test_fast_vehicles_overtake_on_two_lanes_on_the_cpu(oracle):
    """follow_ref.CASES["path1"]'s fleet (vehicle 0 at a 3 m/s target in front, two followers from 6 m/s, 20 m apart) on two lanes, 400 periods:
    every fast vehicle ends ahead of the slow one and back in lane 0 after exactly two changes, nobody touches anybody, every solve Optimal.
    This loop's figures are printed."""
    r, tr, start = LR.cached_overtake(oracle, 2)
    rec = r["rec"]
    ch = [(np.flatnonzero(np.diff(np.concatenate([[0.0], r["lane"][:, b]])) != 0)).tolist() for b in range(3)]
    print("overtake on path1 from samples %s: changes decided in periods %s, last s_along %s m, smallest own-lane gaps %s m, max |e_lane| %s m, "
          "rms e_lane %s m" % (start.tolist(), ch, np.round(r["s_along"], 2), np.round(rec[:, LR.MIN_GAP], 3), np.round(rec[:, LR.MAX_ELANE], 3),
                               np.round(np.sqrt(rec[:, LR.SUM_ELANE2] / rec[:, LR.N]), 3)))
    assert not r["stop"] and np.isfinite(r["state"]).all() and (r["status"] == 0).all()
    assert (r["s_along"][1:] > r["s_along"][0]).all()
    assert (rec[:, LR.LANE] == 0.0).all() and (rec[:, LR.LANE_FROM] == 0.0).all() and (rec[:, LR.OFFSET] == 0.0).all()
    assert rec[:, LR.N_CHANGES].tolist() == [0.0, 2.0, 2.0] and (rec[:, LR.N_CONTACT] == 0.0).all() and (r["gap"] >= 0.0).all()
    assert (r["lane"][:, 0] == 0.0).all() and r["lane"].max() == 1.0 and (r["v_follow"][:, 0] <= 3.0).all()


def test_the_same_fleet_on_one_lane_queues_as_the_follower_shows(oracle):
    """N_LANES = 1, 150 periods: no change, and states, commands, caps and gaps are follow_ref.cpu_platoon's, bit for bit (an offset of 0 leaves the
    waypoints' bits alone): the fast vehicles end queued behind the slow one"""
    r, _, _ = LR.cached_overtake(oracle, 1, steps=150)
    f, _, _ = FR.cached_platoon(oracle, "path1", True)
    for k in ("state", "cmd", "v_follow", "gap"):
        assert r[k].tobytes() == f[k].tobytes(), k
    assert np.array_equal(r["leader"], f["leader"]) and np.array_equal(r["rec"][:, 4:10], f["stat"][:, 0:6])
    assert (r["rec"][:, LR.N_CHANGES] == 0.0).all() and (r["lane"] == 0.0).all() and (r["lane_offset"] == 0.0).all()
    assert (r["s_along"][1:] < r["s_along"][0]).all() and r["leader"][-1].tolist() == [-1, 0, 1]
