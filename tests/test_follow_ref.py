"""CPU side of car following (include/kmpc_follow.h: kmpc_follow_default, kmpc_follow_stat_init, kmpc_follow_fleet): the header's constants against
the Python names, the second export list, both host functions and every argument refusal (no GPU needed: every check comes before the first
device call), properties of the law on the numpy restatement tests/follow_ref.py, and the prototype's platoons as a three-vehicle CPU loop with
and without the stage."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import follow_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1   # KMPC_ERR_ARG
DP = C.POINTER(C.c_double)


def _header():
    txt = open(os.path.join(ROOT, "include", "kmpc_follow.h")).read()
    return txt, re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_constants_and_export_lists():
    from mkz_mpc_path_follower_amd import _lib, ref_traj as RT
    txt, code = _header()
    const = {k: int(v) for k, v in re.findall(r"\b(KMPC_FOLLOW[A-Z_]*)\s*=\s*(\d+)", code)}
    assert [const["KMPC_FOLLOW_" + f.upper()] for f in RT.FOLLOW_FIELDS] == [0, 1, 2, 3, 4] and const["KMPC_FOLLOW_WORDS"] == RT.FOLLOW_WORDS == 8
    assert [const["KMPC_FOLLOWSTAT_" + f.upper()] for f in RT.FOLLOW_STAT_FIELDS] == [0, 1, 2, 3, 4, 5] and const["KMPC_FOLLOWSTAT_WORDS"] == 8
    assert RT.FOLLOW_FIELDS == FR.FIELDS and RT.FOLLOW_STAT_FIELDS == FR.STAT_FIELDS
    declared = sorted(set(re.findall(r"\b(kmpc_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(_lib.EXT_EXPORTS) == ["kmpc_follow_default", "kmpc_follow_fleet", "kmpc_follow_stat_init"]
    L = _lib.load()
    for name in _lib.EXT_EXPORTS:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None and name not in _lib.EXPORTS
    assert len(_lib.EXPORTS) == 60 and L.kmpc_abi_version() == 8
    kmpc_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmpc.h")).read(), flags=re.S)
    assert "kmpc_follow_" not in kmpc_h


def test_host_functions():
    from mkz_mpc_path_follower_amd import _lib, ref_traj as RT
    L = _lib.load()
    r = np.full((3, 8), 7.0)
    assert L.kmpc_follow_default(r.ctypes.data_as(DP), 3) == 0
    assert r[0].tolist() == [5.0, 1.0, 0.7, 0.5, 4.9, 0.0, 0.0, 0.0] and np.array_equal(r, np.tile(FR.DEFAULT_ROW, (3, 1)))
    st = np.full((3, 8), 7.0)
    assert L.kmpc_follow_stat_init(st.ctypes.data_as(DP), 3) == 0 and np.array_equal(st, FR.fresh_stat(3))
    for fn in ("kmpc_follow_default", "kmpc_follow_stat_init"):
        f = getattr(L, fn)
        assert f(None, 1) == ARG and fn.encode() in L.kmpc_last_error(None)
        assert f(r.ctypes.data_as(DP), -1) == ARG and f(None, 0) == 0
    assert np.array_equal(RT.follow_default(), FR.DEFAULT_ROW)
    for bad in (dict(d_min=np.nan), dict(d_min=np.inf), dict(t_headway=-0.1), dict(t_headway=np.inf), dict(a_brake=0.0), dict(a_brake=np.nan),
                dict(k_gap=-1.0), dict(length=-0.1), dict(length=np.nan)):
        with pytest.raises(ValueError):
            RT.check_follow_rows(FR.rows(2, **bad))
    RT.check_follow_rows(FR.rows(2, d_min=-3.0, t_headway=0.0, k_gap=0.0, length=0.0))
    junk = FR.rows(2)
    junk[:, 5:8] = np.nan          # read by nobody
    RT.check_follow_rows(junk)
    with pytest.raises(ValueError):
        RT.check_follow_rows(np.zeros((2, 7)))


def test_argument_checks_answer_before_any_device_call():
    from mkz_mpc_path_follower_amd import _lib
    L = _lib.load()
    p = C.c_void_p(64)   # never dereferenced: every call below is refused on the host
    q = dict(B=2, s=p, ss=4, v=p, vs=8, pid=p, present=p, rows=p, cap=p, out=p, gap=p, leader=p, stat=p)

    def call(**kw):
        a = dict(q, **kw)
        return L.kmpc_follow_fleet(0, a["B"], a["s"], a["ss"], a["v"], a["vs"], a["pid"], a["present"], a["rows"], a["cap"], a["out"], a["gap"],
                                   a["leader"], a["stat"], None)
    for bad in (dict(B=-1), dict(ss=0), dict(ss=-4), dict(vs=0), dict(s=None), dict(v=None), dict(rows=None), dict(cap=None), dict(out=None),
                dict(B=0, ss=0), dict(B=0, vs=0)):
        assert call(**bad) == ARG, bad
        assert b"kmpc_follow_fleet" in L.kmpc_last_error(None)
    # B == 0 succeeds without a launch, whatever the pointers
    assert call(B=0, s=None, v=None, pid=None, present=None, rows=None, cap=None, out=None, gap=None, leader=None, stat=None) == 0


# ---------------------------------------------------------------- the restatement's own properties
def _pair(gap, v_b, v_j, v_cap=30.0, **row):
    """one follower (vehicle 1) `gap` behind vehicle 0 -> follow()'s dict"""
    r = FR.rows(2, **row)
    return FR.follow(np.array([gap + r[1, 4], 0.0]), np.array([v_j, v_b]), None, None, r, np.array([v_cap, v_cap]))


def test_law_is_monotone_in_gap_and_in_the_leaders_speed():
    for row in (dict(), dict(t_headway=0.5), dict(t_headway=0.0, k_gap=0.0), dict(d_min=-2.0, a_brake=2.0)):
        for v_b in (0.0, 3.0, 8.0):
            last = -1.0
            for gap in np.linspace(-3.0, 80.0, 167):
                v = _pair(gap, v_b, 4.0, **row)["v_out"][1]
                assert v >= last and v >= 0.0, (row, v_b, gap)
                last = v
            last = -1.0
            for v_j in np.linspace(0.0, 12.0, 121):
                v = _pair(15.0, v_b, v_j, **row)["v_out"][1]
                assert v >= last, (row, v_b, v_j)
                last = v


def test_settled_gap_is_d_min_plus_headway():
    """v_gap = v_j exactly where gap = D_MIN + T v_b (LENGTH = 0, so that the gap is the arclength difference's own bits).  At equal speeds the
    Gipps arm has the same fixed point, (at + v)^2 = at^2 + v^2 + 2 a T v, up to its rounding: the law returns v_j to within a few ulp there, more
    one metre further back and less one metre closer"""
    for t_h, v in ((1.0, 4.0), (0.5, 3.0), (1.5, 6.0)):
        gap = 5.0 + t_h * v
        o = _pair(gap, v, v, t_headway=t_h, length=0.0)
        assert o["leader"].tolist() == [-1, 0] and o["gap"][1] == gap and o["gap"][0] == np.inf
        w = FR.law(np.array([gap]), np.array([v]), np.array([v]), FR.rows(1, t_headway=t_h, length=0.0), np.array([30.0]))
        assert w["v_gap"][0] == v and abs(w["v_safe"][0] - v) <= 8 * np.spacing(v)
        assert abs(o["v_out"][1] - v) <= 8 * np.spacing(v) and o["bound"][1]
        assert _pair(gap + 1.0, v, v, t_headway=t_h, length=0.0)["v_out"][1] > v > _pair(gap - 1.0, v, v, t_headway=t_h, length=0.0)["v_out"][1]


def test_unbound_cap_keeps_its_bits_and_ties_yield_once():
    d = FR.draw(257, paths=3)
    o = FR.follow(d["s"], d["v"], d["path_id"], d["present"], d["rows"], d["v_cap"])
    free = ~o["bound"]
    assert free.sum() > 20 and o["bound"].sum() > 20 and (o["leader"] < 0).sum() > 20
    assert o["v_out"][free].tobytes() == d["v_cap"][free].tobytes()
    assert (o["v_out"][o["bound"]] < d["v_cap"][o["bound"]]).all()
    has = o["leader"] >= 0
    assert np.isinf(o["gap"][~has]).all() and (o["v_lead"][~has] == 0.0).all() and (o["leader"] != np.arange(257)).all()
    # two vehicles at one arclength: the higher index yields to the lower, which looks further ahead
    t = FR.follow(np.array([10.0, 10.0, 30.0]), np.array([1.0, 2.0, 3.0]), None, None, FR.rows(3), np.full(3, 9.0))
    assert t["leader"].tolist() == [2, 0, -1] and t["gap"][1] == -4.9 and t["stat"][1, 3] == 1.0
    # equal differences cannot arise for one follower on one path except at one arclength: the lowest index leads
    t = FR.follow(np.array([0.0, 7.0, 7.0]), np.ones(3), None, None, FR.rows(3), np.full(3, 9.0))
    assert t["leader"].tolist() == [1, -1, 1]
    # the draw has exact ties among usable vehicles of one path
    ok = FR.usable(d["s"], d["v"], d["path_id"], d["present"])
    keys = list(zip(d["path_id"][ok], d["s"][ok]))
    assert len(set(keys)) < len(keys)


# ---------------------------------------------------------------- the prototype's platoons on the CPU
@pytest.mark.parametrize("case", ["path1", "path2_T05"])
def test_platoon_keeps_its_distance_on_the_cpu(oracle, case):
    """three vehicles, 150 periods: the leader (vehicle 0) at a 3 m/s target, two followers started at 6 m/s behind it, 20 m apart on path1 with the
    default row and 12 m apart on path2 with T = 0.5 s.  Required: no contact in any period and every solve Optimal.  The six-vehicle prototypes gave
    smallest gaps of 7.5 m and 2.05 m; the figures of this loop are printed."""
    r, tr, start = FR.cached_platoon(oracle, case, True)
    print("%s from samples %s: smallest gap per vehicle %s m, last gaps %s m, last speeds %s m/s, bound periods %s, largest closing speed %s m/s"
          % (case, start.tolist(), np.round(r["stat"][:, 4], 3), np.round(r["final_gap"], 3), np.round(r["state"][-1, :, 3], 3),
             r["stat"][:, 2].astype(int).tolist(), np.round(r["stat"][:, 5], 3)))
    assert not r["stop"] and np.isfinite(r["state"]).all()
    assert (r["status"] == 0).all()
    assert (r["stat"][:, 3] == 0).all() and (r["gap"] >= 0.0).all() and (r["final_gap"] >= 0.0).all()
    assert (r["leader"][:, 0] == -1).all() and (r["leader"][:, 1] == 0).all() and (r["leader"][:, 2] == 1).all()
    assert (r["stat"][1:, 2] > 0).all() and (r["v_follow"][:, 0] == 3.0).all()


def test_the_same_fleet_without_the_stage_drives_through_itself(oracle):
    r, _, _ = FR.cached_platoon(oracle, "path1", False)
    print("path1 without the stage: smallest gap seen per vehicle %s m, periods in contact %s" % (np.round(r["stat"][:, 4], 3), r["stat"][:, 3].astype(int).tolist()))
    assert (r["status"] == 0).all() and (r["v_follow"] == np.array([3.0, 6.0, 6.0])).all()
    assert r["gap"].min() < 0.0 and r["stat"][:, 3].sum() > 0
