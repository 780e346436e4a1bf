"""CPU side of the Gauss-Markov stage (kmpc_wander_batch): the header's fields against the Python lists, the neutral row, wander_rows'
conversions and check_wander_rows' refusals, the argument checks (no GPU needed: every check comes before the first device call), the counter
domains, and the restatement of tests/wander_ref.py against the process the header says it is."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import plant_ref as R
import sensor_fault_ref as F
import wander_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1   # KMPC_ERR_ARG


def lib():
    from mkz_mpc_path_follower_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------- header, ABI, defaults, validators
def test_header_enums_match_the_field_lists():
    from mkz_mpc_path_follower_amd import _lib, vehicle_sim as VS
    hdr = open(os.path.join(ROOT, "include", "kmpc.h")).read()
    val = {k: int(v) for k, v in re.findall(r"\b(KMPC_WANDER[A-Z0-9_]*)\s*=\s*(\d+)", hdr)}
    ch = [val["KMPC_WANDER_CH_" + c.upper()] for c in VS.WANDER_CHANNEL_NAMES]
    assert ch == list(range(8)) and val["KMPC_WANDER_CHANNELS"] == VS.WANDER_CHANNELS == W.CHANNELS == 8
    assert (val["KMPC_WANDER_S0"], val["KMPC_WANDER_A"], val["KMPC_WANDER_Q"], val["KMPC_WANDER_WORDS"]) == (W.S0, W.A, W.Q, W.WORDS) == (0, 8, 16, 24)
    assert (val["KMPC_WANDERREC_X"], val["KMPC_WANDERREC_COUNT"], val["KMPC_WANDERREC_WORDS"]) == (W.X, W.COUNT, W.REC_WORDS) == (0, 8, 16)
    assert len(VS.WANDER_FIELDS) == VS.WANDER_WORDS == 24 and len(set(VS.WANDER_FIELDS)) == 24
    for g in ("S0", "A", "Q"):
        for c in VS.WANDER_CHANNEL_NAMES:
            assert VS.WANDER_FIELDS.index("%s_%s" % (g.lower(), c)) == val["KMPC_WANDER_" + g] + val["KMPC_WANDER_CH_" + c.upper()]
    assert [VS.WANDER_RECORD_FIELDS.index("x_" + c) for c in VS.WANDER_CHANNEL_NAMES] == [val["KMPC_WANDERREC_X"] + k for k in ch]
    assert VS.WANDER_RECORD_FIELDS.index("count") == val["KMPC_WANDERREC_COUNT"] and len(VS.WANDER_RECORD_FIELDS) == 9
    # the composed words: the channels' targets are the road row's and the sensor row's words of the same name
    road = {k: int(v) for k, v in re.findall(r"\b(KMPC_ROAD_[A-Z_]*)\s*=\s*(\d+)", hdr)}
    assert {c: road["KMPC_ROAD_" + VS.WANDER_CHANNEL_NAMES[c].upper()] for c in W.ROAD_WORD} == W.ROAD_WORD
    assert int(re.search(r"KMPC_SENSOR_BIAS_X = (\d+)", hdr).group(1)) == 4
    L = lib()
    for name in ("kmpc_wander_default", "kmpc_wander_batch"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.kmpc_abi_version() == 8 and len(_lib.EXPORTS) == 60 and len(L.kmpc_wander_batch.argtypes) == 12


def test_default_rows():
    from mkz_mpc_path_follower_amd import vehicle_sim as VS
    L = lib()
    rows = np.full((3, 24), 7.0)
    dp = C.POINTER(C.c_double)
    assert L.kmpc_wander_default(rows.ctypes.data_as(dp), 3) == 0 and (rows == 0.0).all() and not np.signbit(rows).any()
    assert np.array_equal(VS.wander_default(), W.NEUTRAL) and not W.active(rows).any()
    assert L.kmpc_wander_default(None, 1) == ARG and b"kmpc_wander_default" in L.kmpc_last_error(None)
    assert L.kmpc_wander_default(None, 0) == 0 and L.kmpc_wander_default(rows.ctypes.data_as(dp), -1) == ARG
    assert np.array_equal(VS.wander_rows(5), np.tile(W.NEUTRAL, (5, 1)))      # no argument: every channel off


def test_wander_rows_conversions():
    from mkz_mpc_path_follower_amd import vehicle_sim as VS
    dt = 0.1
    rows = VS.wander_rows(4, dt=dt, sigma=(0.5, 0.5, 0.02, 0.0, 0.3, 0.8, 0.0, 0.1), tau=(np.inf, 0.0, 2.0, 5.0, 10.0, 0.5, 0.0, 30.0),
                          walk=(0, 0, 0, 0.05, 0, 0, 0.002, 0))
    assert rows.shape == (4, 24) and (rows == rows[0]).all()
    s0, a, q = rows[0, 0:8], rows[0, 8:16], rows[0, 16:24]
    assert (s0[0], a[0], q[0]) == (0.5, 1.0, 0.0)                               # tau = inf: a random constant
    assert (s0[1], a[1], q[1]) == (0.5, 0.0, 0.5)                               # tau = 0: white
    for c, tau in ((2, 2.0), (4, 10.0), (5, 0.5), (7, 30.0)):                   # finite tau
        assert a[c] == np.exp(-dt / tau) and q[c] == s0[c] * np.sqrt(1.0 - a[c] * a[c]) and 0.0 < a[c] < 1.0
        assert abs(a[c] * a[c] * s0[c] ** 2 + q[c] ** 2 - s0[c] ** 2) < 1e-15   # stationary: the variance carries over
    for c, r in ((3, 0.05), (6, 0.002)):                                        # a walk
        assert (s0[c], a[c], q[c]) == (0.0, 1.0, r * np.sqrt(dt))
    per = VS.wander_rows(3, sigma=np.arange(24.0).reshape(3, 8), tau=1.0)
    assert np.array_equal(per[:, 0:8], np.arange(24.0).reshape(3, 8)) and (per[1:, 16:24] > 0).all() and per[0, 16] == 0.0
    assert np.array_equal(VS.wander_rows(2, sigma=0.25, tau=np.inf)[:, 0:16], np.tile([0.25] * 8 + [1.0] * 8, (2, 1)))
    t = VS.wander_params(4, device="cpu", sigma=0.2, tau=3.0, dt=0.05)
    assert tuple(t.shape) == (4, 24) and np.array_equal(t.numpy(), VS.wander_rows(4, dt=0.05, sigma=0.2, tau=3.0))
    for bad in (dict(sigma=-0.1), dict(tau=-1.0), dict(walk=-0.1), dict(sigma=np.inf), dict(walk=np.inf), dict(sigma=np.nan), dict(tau=np.nan),
                dict(sigma=np.zeros(4)), dict(tau=np.zeros((3, 8))), dict(sigma=0.1, walk=0.1), dict(dt=0.0), dict(dt=np.inf)):
        with pytest.raises(ValueError):
            VS.wander_rows(4, **bad)


def test_check_wander_rows_refusals():
    from mkz_mpc_path_follower_amd import vehicle_sim as VS
    ok = W.stationary_rows(4, [0.5, 0.5, 0.02, 0.1, 0.3, 0.8, 0.01, 0], [0.99, 0.9, 0.5, 0, 0.95, 0.8, 1, 0.3])
    assert VS.check_wander_rows(ok) is not None and VS.check_wander_rows(W.mixed_case()["rows"]) is not None
    for w, v in ((0, -0.1), (7, np.inf), (3, np.nan), (8, -0.01), (9, 1.0001), (15, np.nan), (12, np.inf), (16, -1e-9), (23, np.inf), (20, np.nan)):
        rows = ok.copy()
        rows[2, w] = v
        with pytest.raises(ValueError):
            VS.check_wander_rows(rows)
    for shape in ((4, 16), (24,), (2, 3, 24)):
        with pytest.raises(ValueError):
            VS.check_wander_rows(np.zeros(shape))
    for kw in (dict(B=5), dict(seed=-1), dict(seed=2 ** 64), dict(id_base=-1)):
        with pytest.raises(ValueError):
            VS.Wander(**dict(dict(B=4, rows=ok, device="cpu"), **kw))
    w = VS.Wander(4, ok, device="cpu")
    assert w.sensor_active and w.road_active and tuple(w.x.shape) == (4, 8) and w.x.data_ptr() == w.rec.data_ptr()
    only_free = np.zeros((4, 24)); only_free[:, 7] = 1.0
    w = VS.Wander(4, only_free, device="cpu")
    assert not w.sensor_active and not w.road_active
    with pytest.raises(RuntimeError):
        w.step(0)                                                                # no CPU fallback


# ---------------------------------------------------------------- argument checks without a GPU: one test per bad argument
P = C.c_void_p(64)     # never dereferenced: every call below is refused on the host
Q_ = C.c_void_p(4096)
GOOD = dict(B=4, rows=P, rec=P, period=0, id_base=0, sb=P, so=Q_, rb=P, ro=Q_)


def call(**kw):
    a = dict(GOOD, **kw)
    return lib().kmpc_wander_batch(0, a["B"], a["rows"], a["rec"], 1, a["period"], a["id_base"], a["sb"], a["so"], a["rb"], a["ro"], None)


def refused(**kw):
    L = lib()
    assert L.kmpc_wander_default(None, 1) == ARG and b"kmpc_wander_batch" not in L.kmpc_last_error(None)   # another call's text: the refusal below writes its own
    assert call(**kw) == ARG, kw
    msg = L.kmpc_last_error(None)
    assert msg and b"kmpc_wander_batch" in msg, msg


def test_negative_B_is_refused():
    refused(B=-1)


def test_negative_period_is_refused():
    refused(period=-1)


def test_negative_id_base_is_refused():
    refused(id_base=-1)


def test_period_two_to_the_62_is_refused():
    refused(period=2 ** 62)
    refused(period=2 ** 63 - 1)
    assert call(B=0, period=2 ** 62 - 1) == 0


def test_null_rows_are_refused():
    refused(rows=None)


def test_null_record_is_refused():
    refused(rec=None)


def test_half_a_pair_is_refused():
    for kw in (dict(sb=None), dict(so=None), dict(rb=None), dict(ro=None), dict(sb=None, ro=None)):
        refused(**kw)


def test_out_equal_base_is_refused():
    refused(so=P)
    refused(ro=P)
    refused(sb=None, so=None, ro=P)


def test_empty_batch_succeeds_without_a_launch():
    assert call(B=0) == 0 and call(B=0, rows=None, rec=None) == 0 and call(B=0, sb=None, so=None, rb=None, ro=None) == 0


# ---------------------------------------------------------------- counter domains
def test_counter_domains_are_apart():
    """for the same (seed, gid, period) the two wander draws, the measurement draw and the fault draw are four different Philox counters: they differ
    in the top two bits of the last word, which a period below 2^62 leaves clear"""
    M = R.M32
    for seed, gid, period in ((9, 5, 3), (0x9E3779B97F4A7C15, 2 ** 32 + 1, 2 ** 33 + 7), (0, 0, 0), (1, 2 ** 40, 2 ** 62 - 1)):
        key = (seed & M, (seed >> 32) & M)
        ctr = lambda top: (gid & M, (gid >> 32) & M, period & M, ((period >> 32) & M) ^ top)
        w0, w1 = W.words(seed, gid, period, 0), W.words(seed, gid, period, 1)
        assert w0 == R.philox4x32_10(ctr(0x40000000), key) and w1 == R.philox4x32_10(ctr(0xC0000000), key)
        meas, fault = R.philox4x32_10(ctr(0), key), R.philox4x32_10(ctr(0x80000000), key)
        assert len({w0, w1, meas, fault}) == 4
        assert np.array_equal((np.array(fault, dtype=np.float64) + 0.5) * 2.0 ** -32, F.fault_uniforms(seed, gid, period))
        n = W.normals(seed, gid, period)
        assert n.shape == (8,) and np.isfinite(n).all()
        m = R.normals(seed, gid, period)
        assert not np.isin(n, m).any() and len(set(n.tolist())) == 8
        assert ((period >> 32) & M) < 2 ** 30
    # an array of vehicle ids is the loop over them, across the 2^32 boundary
    gids = np.arange(2 ** 32 - 3, 2 ** 32 + 3, dtype=np.uint64)
    assert np.array_equal(W.normals(7, gids, 11), np.array([W.normals(7, int(g), 11) for g in gids]))
    with pytest.raises(AssertionError):
        W.words(1, 0, 2 ** 62, 0)


# ---------------------------------------------------------------- the restatement alone
def test_off_constant_walk_and_reset_in_the_restatement():
    c = W.mixed_case()
    h = W.run(c["rows"], c["seed"], range(W.CASE_PERIODS), id_base=3, sensor_base=c["sensor"], road_base=c["road"])
    k = c["kind"]
    off = k >= 4
    assert np.array_equal(W.active(c["rows"]), ~off) and off[120:130].all() and off[130:140, 0:4].all() and off[140:150, 4:8].all()
    x = h["x"]
    assert (x[:, off] == 0.0).all() and not np.signbit(x[:, off]).any() and (x[1:, ~off] != 0.0).all()
    assert (x[0, k == 3] == 0.0).all() and (x[0, k <= 2] != 0.0).all()                   # a walk starts at S0 * n = 0 (of either sign)
    assert (x[1:, k == 2] == x[0, k == 2]).all()                                         # A = 1, Q = 0 keeps the first draw
    assert (h["count"] == np.arange(1, W.CASE_PERIODS + 1)[:, None]).all()
    # off: the composed word is the base's, bit for bit (a -0.0 stays -0.0); active: base + x
    so, ro = h["sensor_out"], h["road_out"]
    assert np.array_equal(so[:, :, 0:4], np.broadcast_to(c["sensor"][:, 0:4], so[:, :, 0:4].shape))
    sb = np.broadcast_to(c["sensor"][:, 4:8], so[:, :, 4:8].shape)
    assert np.array_equal(so[:, :, 4:8][:, off[:, 0:4]].view(np.int64), sb[:, off[:, 0:4]].copy().view(np.int64))
    assert np.array_equal(so[:, :, 4:8], np.where(off[:, 0:4], sb, sb + x[:, :, 0:4]))
    for w_ in (0, 1, 5, 6, 7):
        assert (ro[:, :, w_] == c["road"][:, w_]).all()
    for ch, w_ in W.ROAD_WORD.items():
        rb = np.broadcast_to(c["road"][:, w_], ro[:, :, w_].shape)
        assert np.array_equal(ro[:, :, w_].view(np.int64), np.where(off[:, ch], rb, rb + x[:, :, ch]).view(np.int64))
    assert np.signbit(ro[:, 50:60][:, off[50:60, 4]][..., 2]).all()
    # neutral rows: nothing moves
    n = W.run(np.tile(W.NEUTRAL, (6, 1)), 5, range(3), sensor_base=c["sensor"][:6], road_base=c["road"][:6])
    assert (n["x"] == 0.0).all() and np.array_equal(n["sensor_out"][2].view(np.int64), c["sensor"][:6].view(np.int64))
    assert np.array_equal(n["road_out"][2].view(np.int64), c["road"][:6].view(np.int64))
    # a poisoned COUNT: fresh again, the others untouched; words 9 ... 15 come back as read
    rec = h["rec"].copy()
    rec[:, 9:16] = np.arange(7.0)
    bad = rec.copy()
    bad[3, W.COUNT], bad[4, W.COUNT], bad[5, W.COUNT] = np.nan, -1.0, np.inf
    o, ref = W.step(c["rows"], bad, c["seed"], 99, 3), W.step(c["rows"], rec, c["seed"], 99, 3)
    fresh = W.step(c["rows"], np.zeros_like(rec), c["seed"], 99, 3)
    assert (o["rec"][3:6, W.COUNT] == 1).all() and np.array_equal(o["x"][3:6], fresh["x"][3:6]) and o["fresh"][3:6].all()
    keep = np.ones(W.CASE_B, bool); keep[3:6] = False
    assert np.array_equal(o["rec"][keep], ref["rec"][keep]) and (o["rec"][:, 9:16] == np.arange(7.0)).all() and (ref["rec"][:, W.COUNT] == 17).all()


def test_the_specification_produces_the_process_it_claims():
    """The reference alone: seed 7, B = 2048, 64 periods from a fresh record, S0 = (0.5, 0.5, 0.02, 0.1, 0.3, 0.8, 0.01, 0),
    A = (0.99, 0.9, 0.5, 0, 0.95, 0.8, 1, 0.3), Q = S0 sqrt(1 - A^2).  Per active channel over the fleet at the last period: |std / S0 - 1|,
    |mean| / S0 and |E[x_k x_(k-1)] / S0^2 - A| below 4 / sqrt(B) = 0.088 (the standard error of each is at most about 1.4 / sqrt(B)); the standard
    deviation at period 0 too; every cross-channel correlation below 6 / sqrt(B) = 0.133 (21 pairs); channel 7, off, exactly 0 throughout.
    The restatement gives 0.025 (std), 0.037 (std at period 0), 0.044 (mean), 0.021 (lag 1), 0.091 (cross-channel)."""
    B, K = 2048, 64
    s0 = np.array([0.5, 0.5, 0.02, 0.1, 0.3, 0.8, 0.01, 0.0])
    a = np.array([0.99, 0.9, 0.5, 0.0, 0.95, 0.8, 1.0, 0.3])
    x = W.run(W.stationary_rows(B, s0, a), 7, range(K))["x"]
    act = s0 > 0.0
    assert act.sum() == 7 and (x[:, :, 7] == 0.0).all() and not np.signbit(x[:, :, 7]).any()
    last, prev = x[K - 1][:, act], x[K - 2][:, act]
    std = np.abs(last.std(0) / s0[act] - 1.0)
    std0 = np.abs(x[0][:, act].std(0) / s0[act] - 1.0)
    mean = np.abs(last.mean(0)) / s0[act]
    lag = np.abs((last * prev).mean(0) / s0[act] ** 2 - a[act])
    cross = np.abs(np.corrcoef(last.T) - np.eye(7))
    print("std %.3f, std at period 0 %.3f, mean %.3f, lag 1 %.3f, cross-channel %.3f" % (std.max(), std0.max(), mean.max(), lag.max(), cross.max()))
    bound = 4.0 / np.sqrt(B)
    assert (std < bound).all() and (std0 < bound).all() and (mean < bound).all() and (lag < bound).all()
    assert (cross < 6.0 / np.sqrt(B)).all()
    assert (x[:, :, 6] == x[0, :, 6]).all()                                     # A = 1, Q = 0: the first draw for ever


def test_a_walk_spreads_with_the_square_root_of_time():
    """S0 = 0, A = 1, Q = 0.1 in channel 2, B = 2048: the first value is 0 (S0 * n), after k further calls the standard deviation is Q sqrt(k).
    Bound 4 / sqrt(B) on the ratio, as above (the standard error of a standard deviation is 0.71 / sqrt(B))."""
    B = 2048
    rows = np.zeros((B, 24))
    rows[:, W.A + 2], rows[:, W.Q + 2] = 1.0, 0.1
    x = W.run(rows, 11, range(26))["x"][:, :, 2]
    assert (x[0] == 0.0).all()
    for k in (1, 9, 25):
        assert abs(x[k].std() / (0.1 * np.sqrt(k)) - 1.0) < 4.0 / np.sqrt(B), k
