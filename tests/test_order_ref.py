"""CPU side of the ordered leader search (include/kmpc_order.h: kmpc_order_bytes, kmpc_order_fleet, kmpc_order_follow_fleet,
kmpc_order_lane_step_fleet): the fifth export list, the host function, every argument refusal (no GPU needed: every check comes before the first
device call), the numpy restatement tests/order_ref.py against the pair searches of follow_ref and lanes_ref, and the search= argument."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import follow_ref as FR
import lanes_ref as LR
import order_ref as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1   # KMPC_ERR_ARG
NAMES = ["kmpc_order_bytes", "kmpc_order_fleet", "kmpc_order_follow_fleet", "kmpc_order_lane_step_fleet"]


def _code(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_header_and_export_lists():
    from mkz_mpc_path_follower_amd import _lib
    declared = sorted(set(re.findall(r"\b(kmpc_[a-z0-9_]+)\s*\(", _code("kmpc_order.h"))))
    assert declared == sorted(_lib.ORDER_EXPORTS) == NAMES
    L = _lib.load()
    for name in NAMES:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None
        assert name not in _lib.EXPORTS + _lib.EXT_EXPORTS + _lib.LANE_EXPORTS + _lib.RANGE_EXPORTS
    assert (len(_lib.EXPORTS), len(_lib.EXT_EXPORTS), len(_lib.LANE_EXPORTS), len(_lib.RANGE_EXPORTS)) == (60, 3, 4, 3)
    assert L.kmpc_abi_version() == 8
    for other in ("kmpc.h", "kmpc_follow.h", "kmpc_lanes.h", "kmpc_range.h"):
        assert "kmpc_order" not in _code(other) and "KMPC_ORDER" not in _code(other), other
    # the argument lists are the pair searches' with the order's words behind them
    assert L.kmpc_order_follow_fleet.argtypes[:14] == L.kmpc_follow_fleet.argtypes[:14] and len(L.kmpc_order_follow_fleet.argtypes) == 16
    assert L.kmpc_order_lane_step_fleet.argtypes[:22] == L.kmpc_lane_step_fleet.argtypes[:22] and len(L.kmpc_order_lane_step_fleet.argtypes) == 27


def _bytes(L, B, lanes_max):
    n = C.c_int64(-7)
    assert L.kmpc_order_bytes(B, lanes_max, C.byref(n)) == 0
    return n.value


def test_order_bytes_is_monotone_and_checks_its_arguments():
    from mkz_mpc_path_follower_amd import _lib
    L = _lib.load()
    n = C.c_int64()
    for bad in ((-1, 0), (4, -1), (4, 33)):
        assert L.kmpc_order_bytes(bad[0], bad[1], C.byref(n)) == ARG and b"kmpc_order_bytes" in L.kmpc_last_error(None)
    assert L.kmpc_order_bytes(4, 0, None) == ARG
    sizes = [0, 1, 2, 255, 256, 257, 2048, 2049, 70001, 262144, 2 ** 21, 2 ** 21 + 1, 3 * 2 ** 20, 2 ** 24, 2 ** 31 - 1]
    table = np.array([[_bytes(L, B, m) for m in range(33)] for B in sizes], dtype=np.int64)
    assert (table >= 0).all() and (table[0] == 0).all() and (table[1:] > 0).all()
    assert (np.diff(table, axis=0) >= 0).all() and (np.diff(table, axis=1) >= 0).all()
    assert (np.diff(table[sizes.index(256):], axis=1) > 0).all()        # from one workgroup of positions on, every lane's tables take room
    # the sort's share: three words and a fraction per vehicle; a lane's tables: two int32 per vehicle and lane
    assert 16 * 262144 <= table[sizes.index(262144), 0] <= 18 * 262144
    assert 8 * 262144 <= table[sizes.index(262144), 1] - table[sizes.index(262144), 0] <= 8 * 262144 + 65536


def test_argument_checks_answer_before_any_device_call():
    from mkz_mpc_path_follower_amd import _lib
    L = _lib.load()
    p, p2 = C.c_void_p(64), C.c_void_p(4096)   # never dereferenced: every call below is refused on the host
    big = 1 << 40

    def order(**kw):
        a = dict(dict(B=2, s=p, ss=4, v=p, vs=8, pid=p, pr=p, out=p, cnt=p, ws=p, nb=big), **kw)
        return L.kmpc_order_fleet(0, a["B"], a["s"], a["ss"], a["v"], a["vs"], a["pid"], a["pr"], a["out"], a["cnt"], a["ws"], a["nb"], None)
    for bad in (dict(B=-1), dict(ss=0), dict(vs=0), dict(vs=-8), dict(nb=0), dict(nb=_bytes(L, 2, 0) - 1), dict(nb=-1), dict(s=None), dict(v=None),
                dict(out=None), dict(ws=None), dict(B=0, ss=0), dict(B=0, nb=-1)):
        assert order(**bad) == ARG, bad
        assert b"kmpc_order_fleet" in L.kmpc_last_error(None)
    assert order(nb=_bytes(L, 2, 0), pid=None, pr=None, cnt=None, s=None) == ARG      # the exact size passes the size check; the NULL is caught
    assert order(B=0, s=None, v=None, out=None, ws=None, cnt=None, pid=None, pr=None, nb=0) == 0

    def follow(**kw):
        a = dict(dict(B=2, s=p, ss=4, v=p, vs=8, pid=p, pr=p, rows=p, cap=p, out=p, gap=p, lead=p, stat=p, order=p), **kw)
        return L.kmpc_order_follow_fleet(0, a["B"], a["s"], a["ss"], a["v"], a["vs"], a["pid"], a["pr"], a["rows"], a["cap"], a["out"], a["gap"],
                                         a["lead"], a["stat"], a["order"], None)
    for bad in (dict(B=-1), dict(ss=0), dict(vs=0), dict(s=None), dict(v=None), dict(rows=None), dict(cap=None), dict(out=None), dict(order=None),
                dict(B=0, vs=0)):
        assert follow(**bad) == ARG, bad
        assert b"kmpc_order_follow_fleet" in L.kmpc_last_error(None)
    assert follow(B=0, s=None, v=None, rows=None, cap=None, out=None, order=None) == 0

    def lanes(**kw):
        a = dict(dict(B=2, k=0, dt=0.1, s=p, ss=4, e=p, es=4, v=p, vs=8, pid=p, pr=p, fr=p, lr=p, cap=p, out=p, oin=p, oout=p2, rec=p, gap=p, lead=p,
                      nbr=p, order=p, lm=2, ws=p, nb=big), **kw)
        return L.kmpc_order_lane_step_fleet(0, a["B"], a["k"], a["dt"], a["s"], a["ss"], a["e"], a["es"], a["v"], a["vs"], a["pid"], a["pr"], a["fr"],
                                            a["lr"], a["cap"], a["out"], a["oin"], a["oout"], a["rec"], a["gap"], a["lead"], a["nbr"], a["order"],
                                            a["lm"], a["ws"], a["nb"], None)
    for bad in (dict(B=-1), dict(k=-1), dict(ss=0), dict(es=0), dict(vs=0), dict(dt=0.0), dict(dt=-0.1), dict(dt=np.nan), dict(dt=np.inf),
                dict(lm=-1), dict(lm=33), dict(nb=0), dict(nb=_bytes(L, 2, 2) - 1), dict(B=256, lm=3, nb=_bytes(L, 256, 2)), dict(s=None), dict(e=None),
                dict(v=None), dict(fr=None), dict(lr=None), dict(cap=None), dict(out=None), dict(oin=None), dict(oout=None), dict(rec=None),
                dict(order=None), dict(ws=None), dict(oout=p), dict(B=0, k=-1), dict(B=0, lm=40)):
        assert lanes(**bad) == ARG, bad
        assert b"kmpc_order_lane_step_fleet" in L.kmpc_last_error(None)
    assert lanes(B=0, s=None, e=None, v=None, fr=None, lr=None, cap=None, out=None, oin=None, oout=None, rec=None, order=None, ws=None, nb=0) == 0


# ---------------------------------------------------------------- the restatement against the pair searches
SIZES = (1, 2, 63, 65, 257, 1000)


def _check_follow(d, tag):
    l0, d0 = FR.leaders(d["s"], d["v"], d["path_id"], d["present"])
    l1, d1 = OR.search(d["s"], d["v"], d["path_id"], d["present"])
    assert np.array_equal(l0, l1), (tag, np.flatnonzero(l0 != l1)[:5])
    assert np.array_equal(d0, d1), tag


def _check_lanes(d, tag):
    e = LR.step_draw(d, 0)
    win, dif = OR.lane_searches(d)
    assert np.array_equal(win, e["winners"]), (tag, np.argwhere(win != e["winners"])[:5])
    # the differences reach the outputs as gaps: own-ahead's through gap, the sides' through nbr
    fr = d["follow_rows"]
    with np.errstate(all="ignore"):
        has = win[:, 0] >= 0
        assert np.array_equal((dif[:, 0] - fr[:, 4])[has], e["gap"][has]), tag
        for i, col in ((1, 0), (2, 1), (3, 2), (4, 3)):
            has = win[:, i] >= 0
            assert np.array_equal((dif[:, i] - fr[:, 4])[has], e["nbr"][has, col, 0]), (tag, i)


@pytest.mark.parametrize("B", SIZES)
def test_ordered_search_is_the_pair_search(B):
    for kind in OR.KINDS:
        for paths in (0, 3):
            for seed in range(2):
                _check_follow(OR.draw(kind, B, seed, paths), (kind, B, seed, paths))


@pytest.mark.parametrize("B", SIZES)
def test_ordered_lane_searches_are_the_pair_searches(B):
    for kind in OR.KINDS:
        for paths in (0, 3):
            _check_lanes(OR.draw(kind, B, 0, paths, lanes=True), (kind, B, paths))


def test_adversarial_draws_of_forty():
    for seed in range(200):
        _check_follow(OR.draw("adversarial", 40, seed, 0), ("adversarial", seed))
        if seed < 40:
            _check_lanes(OR.draw("adversarial", 40, seed, 2, lanes=True), ("adversarial lanes", seed))


def test_the_order_is_a_permutation_with_the_stated_keys():
    for kind in OR.KINDS:
        d = OR.draw(kind, 257, 1, 3)
        o, n = OR.order(d["s"], d["v"], d["path_id"], d["present"])
        ok = FR.usable(d["s"], d["v"], d["path_id"], d["present"])
        assert sorted(o.tolist()) == list(range(257)) and n == int(ok.sum())
        assert ok[o[:n]].all() and not ok[o[n:]].any() and (np.diff(o[n:]) > 0).all()
        pid, s = d["path_id"][o[:n]].astype(np.int64), d["s"][o[:n]]
        for a in range(n - 1):
            key_a, key_b = (pid[a], s[a] + 0.0, -o[a]), (pid[a + 1], s[a + 1] + 0.0, -o[a + 1])
            assert key_a < key_b, (kind, a)


def test_search_argument():
    from mkz_mpc_path_follower_amd import ref_traj as RT
    import inspect
    assert inspect.signature(RT.Follower.__init__).parameters["search"].default == "pairs"
    sig = inspect.signature(RT.Lanes.__init__).parameters
    assert sig["search"].default == "pairs" and sig["lanes_max"].default is None
    assert RT.check_search("pairs") == "pairs" and RT.check_search("sorted") == "sorted"
    for bad in ("bogus", "auto", None, 1):
        with pytest.raises(ValueError):
            RT.check_search(bad)
