"""CPU side of the sensor-fault stage: the restatement of tests/sensor_fault_ref.py against plant_ref.sense and against itself (the committed
case has the branches it promises, a schedule leaves the chain alone, held values are the last delivered ones, the chain's silent share), the
header's fields, the symbols and their argument checks (no GPU needed: every check comes before the first device call), the Python validators,
and one-vehicle CPU loops through an outage: held fix against dead reckoning, and the blind stop."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import plant_ref as R
import sensor_fault_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("kmpc_sense_faults_default", "kmpc_sense_faults_batch")
ARG = -1   # KMPC_ERR_ARG


@pytest.fixture(scope="module")
def case_run():
    case = F.committed_case()
    return case, F.run_case(case)


def test_committed_case_has_the_branches_it_promises(case_run):
    """300 vehicles x 40 periods, six groups of 50.  Counted in the restatement: silent vehicle-periods per source 3614 / 3556 / 3713, regains
    593 / 533 / 589, all three silent at once 1543, a scheduled window on top of a silent chain 381, outliers 1541, 50 vehicles that go blind
    (1187 vehicle-periods), 300 fresh calls.  The floors are about half of each: what the rows' probabilities give with a wide margin."""
    case, h = case_run
    g = case["group"]
    assert [int((g == k).sum()) for k in range(6)] == [50] * 6
    f = case["faults"]
    assert (f[g == 0] == F.NEUTRAL).all() and (f[g == 5, F.P_REGAIN:F.P_REGAIN + 3] == 0.0).all() and (f[g == 3, F.P_LOSE:F.P_LOSE + 3] == 0.0).all()
    assert set(np.unique(f[g == 4, F.MAX_AGE])) == {0.0, 1.0, 2.0, 3.0, 4.0, 5.0} and np.isinf(f[g != 4, F.MAX_AGE]).all()
    sil, ch = h["silent"], h["chain"]
    p = np.arange(F.CASE_PERIODS)[:, None, None]
    frm, ln = f[None, :, F.WIN_FROM:F.WIN_FROM + 3], f[None, :, F.WIN_LEN:F.WIN_LEN + 3]
    sched = (ln > 0) & (p >= frm) & (p < frm + ln)
    counts = dict(silent=sil.sum((0, 1)), regained=(sil[:-1] & ~sil[1:]).sum((0, 1)), all_three=sil.all(2).sum(), sched_on_chain=(sched & ch).sum(),
                  sched_alone=(sched & ~ch & sil).sum(), outliers=h["outlier"].sum(), blind_vehicles=h["blind"].any(0).sum(), blind=h["blind"].sum(),
                  fresh=h["fresh"].sum())
    print(counts)
    assert (counts["silent"] >= 1800).all() and (counts["regained"] >= 250).all() and counts["all_three"] >= 700
    assert counts["sched_on_chain"] >= 150 and counts["sched_alone"] >= 800 and counts["outliers"] >= 700
    assert counts["blind_vehicles"] >= 30 and counts["blind"] >= 500 and counts["fresh"] == F.CASE_B and h["fresh"][0].all() and not h["fresh"][1:].any()
    # per group: only the groups that may be silent are, outliers only where a fix was delivered, the sticky group never regains
    assert not sil[:, (g == 0) | (g == 3)].any() and not h["outlier"][:, (g != 3) & (g != 4)].any() and not (h["outlier"] & sil[:, :, 0]).any()
    stick = sil[:, g == 5]
    assert not (stick[:-1] & ~stick[1:]).any() and stick[-1].sum() >= 100
    assert set(np.unique(h["flags"][:, g == 0])) == {0, F.F_FRESH}


def test_neutral_row_is_the_plain_sensor_bit_for_bit(case_run):
    case, h = case_run
    g = case["group"] == 0
    for p in range(F.CASE_PERIODS):
        want = R.sense(case["states"][p], case["sensor"], case["seed"], p, id_base=case["id_base"])
        assert np.array_equal(h["z"][p][g], want[g]) and np.array_equal(h["held"][p][g], want[g]), p
        assert np.array_equal(h["measured"][p][~h["outlier"][p]], want[~h["outlier"][p]])       # every non-outlier fix is the plain sensor's too
    neutral = F.run_case(case, periods=6, faults=np.tile(F.NEUTRAL, (F.CASE_B, 1)))
    assert np.array_equal(neutral["z"], neutral["held"]) and (neutral["flags"][1:] == 0).all() and (neutral["rec"][-1][:, F.COUNT] == 6).all()


def test_a_schedule_leaves_the_chain_where_it_would_have_been(case_run):
    """the same rows without their windows: the stored chain is the same in every period, and silence is chain OR window"""
    case, h = case_run
    bare = case["faults"].copy()
    bare[:, F.WIN_LEN:F.WIN_LEN + 3] = 0.0
    hb = F.run_case(case, faults=bare)
    assert np.array_equal(hb["chain"], h["chain"]) and np.array_equal(hb["rec"][:, :, F.CHAIN], h["rec"][:, :, F.CHAIN])
    assert np.array_equal(hb["silent"], hb["chain"]) and (h["silent"] >= h["chain"]).all() and (h["silent"] != h["chain"]).sum() >= 800
    assert np.array_equal(h["rec"][:, :, F.CHAIN], (h["chain"] * np.array([1, 2, 4])).sum(2))


def test_held_values_are_the_last_delivered_ones(case_run):
    """bookkeeping of its own: per channel the held value is the measured value of the latest period in which the channel's source delivered; ages,
    counters and the longest silence follow from the silent pattern alone"""
    case, h = case_run
    K, B = F.CASE_PERIODS, F.CASE_B
    last = np.zeros((B, 4))
    age, longest = np.zeros((B, 3)), np.zeros((B, 3))
    for p in range(K):
        sil_c = h["silent"][p][:, F.SOURCE_OF]
        last = np.where(sil_c, last, h["measured"][p])
        assert np.array_equal(h["held"][p], last) and np.array_equal(h["rec"][p][:, 0:4], last), p
        assert np.array_equal(np.isnan(h["z"][p]), sil_c) and np.array_equal(h["z"][p][~sil_c], h["measured"][p][~sil_c])
        age = np.where(h["silent"][p], age + 1, 0)
        longest = np.maximum(longest, age)
        assert np.array_equal(h["rec"][p][:, F.AGE:F.AGE + 3], age) and np.array_equal(h["rec"][p][:, F.LONGEST:F.LONGEST + 3], longest)
        assert np.array_equal(h["blind"][p], (age > case["faults"][:, F.MAX_AGE:F.MAX_AGE + 1]).any(1))
    assert np.array_equal(h["rec"][-1][:, F.N_SILENT:F.N_SILENT + 3], h["silent"].sum(0)) and np.array_equal(h["rec"][-1][:, F.N_OUTLIER], h["outlier"].sum(0))
    assert (h["rec"][-1][:, F.COUNT] == K).all()


def test_poisoned_record_is_taken_as_fresh():
    case = F.committed_case()
    rec = F.run_case(case, periods=5)["rec"][-1]
    bad = rec.copy()
    bad[3, F.COUNT], bad[4, F.COUNT], bad[5, F.CHAIN], bad[6, F.CHAIN], bad[7, F.COUNT] = np.nan, -1.0, 8.0, 2.5, np.inf
    o = F.sense_faults(case["states"][5], case["sensor"], case["faults"], bad, case["seed"], 5, case["id_base"])
    ref = F.sense_faults(case["states"][5], case["sensor"], case["faults"], rec, case["seed"], 5, case["id_base"])
    hit = np.zeros(F.CASE_B, bool)
    hit[3:8] = True
    assert (o["flags"][hit] == F.F_FRESH | F.F_RESET).all() and (o["rec"][hit, F.COUNT] == 1).all() and not np.isnan(o["z"][hit]).any()
    assert (o["rec"][hit, F.AGE:] == 0).all()
    for k in ("rec", "z", "held", "flags", "blind"):
        assert np.array_equal(o[k][~hit], ref[k][~hit], equal_nan=True), k


def test_chain_statistics():
    """P_LOSE 0.05, P_REGAIN 0.2 on all three sources, 300 vehicles x 200 periods from fresh records.  The stationary silent share is
    pi = P_LOSE / (P_LOSE + P_REGAIN) = 0.2.  The chain's autocorrelation at lag t is lambda^t with lambda = 1 - P_LOSE - P_REGAIN = 0.75, so
      - a start in the delivering state (the fresh call delivers) lowers the expected share over n = 200 periods by pi * sum_t lambda^t / n
        = 0.2 * 4 / 200 = 0.004: the expectation is 0.196;
      - the variance of one vehicle's share is pi (1 - pi) / n * (1 + lambda) / (1 - lambda) = 0.16 / 200 * 7 = 0.0056, and of the mean over 300
        independent vehicles 1.87e-5: a standard deviation of 0.0043 per source.
    Bound: |share - 0.2| <= 0.004 + 5 * 0.0043 = 0.0255 for each source.  The restatement gives 0.1993 / 0.2021 / 0.2034 (GPS / IMU / SPD)
    with this seed."""
    B, K = 300, 200
    rows = np.tile(F.NEUTRAL, (B, 1))
    rows[:, F.P_LOSE:F.P_LOSE + 3], rows[:, F.P_REGAIN:F.P_REGAIN + 3] = 0.05, 0.2
    rec = np.zeros((B, F.WORDS))
    n = np.zeros(3)
    for p in range(K):
        d = F.decide(rows, rec, 12345, p, 0)
        n += d["silent"].sum(0)
        rec = rec.copy()
        rec[:, F.COUNT], rec[:, F.CHAIN] = p + 1.0, (d["chain"] * np.array([1, 2, 4])).sum(1)
    share = n / (B * K)
    print("silent share per source:", share)
    assert (np.abs(share - 0.2) <= 0.0255).all()


def test_fault_draw_is_not_the_noise_draw():
    u = F.fault_uniforms(9, 5, 3)
    M = R.M32
    w = R.philox4x32_10((5, 0, 3, 0x80000000), (9, 0))
    assert np.array_equal(u, (np.array(w, dtype=np.float64) + 0.5) * 2.0 ** -32) and (u > 0).all() and (u < 1).all()
    assert w != R.philox4x32_10((5, 0, 3, 0), (9, 0)) and M == 0xFFFFFFFF


# ---------------------------------------------------------------- header, ABI, validators
def test_header_fields_flags_and_defaults():
    from mkz_mpc_path_follower_amd import _lib, vehicle_sim as VS
    hdr = open(os.path.join(ROOT, "include", "kmpc.h")).read()
    val = {k: int(v) for k, v in re.findall(r"\b(KMPC_FAULT[A-Z_]*)\s*=\s*(\d+)", hdr)}
    src = ("GPS", "IMU", "SPD")
    for name, first in (("P_LOSE", F.P_LOSE), ("P_REGAIN", F.P_REGAIN), ("WIN_FROM", F.WIN_FROM), ("WIN_LEN", F.WIN_LEN)):
        assert [val["KMPC_FAULT_%s_%s" % (name, s)] for s in src] == [first, first + 1, first + 2]
    assert (val["KMPC_FAULT_P_OUTLIER"], val["KMPC_FAULT_OUTLIER_SIGMA"], val["KMPC_FAULT_MAX_AGE"], val["KMPC_FAULT_WORDS"]) == (12, 13, 14, 16)
    assert [val["KMPC_FAULTREC_HELD_" + c] for c in ("X", "Y", "PSI", "V")] == [0, 1, 2, 3]
    assert (val["KMPC_FAULTREC_COUNT"], val["KMPC_FAULTREC_CHAIN"], val["KMPC_FAULTREC_N_OUTLIER"], val["KMPC_FAULTREC_WORDS"]) == (F.COUNT, F.CHAIN, F.N_OUTLIER, 16)
    for name, first in (("AGE", F.AGE), ("N_SILENT", F.N_SILENT), ("LONGEST", F.LONGEST)):
        assert [val["KMPC_FAULTREC_%s_%s" % (name, s)] for s in src] == [first, first + 1, first + 2]
    assert tuple(val["KMPC_FAULT_FLAG_SILENT_" + s] for s in src) == F.F_SILENT
    assert [val["KMPC_FAULT_FLAG_" + k] for k in ("OUTLIER", "BLIND", "FRESH", "RESET")] == [F.F_OUTLIER, F.F_BLIND, F.F_FRESH, F.F_RESET]
    assert (VS.FAULT_SILENT_GPS, VS.FAULT_SILENT_IMU, VS.FAULT_SILENT_SPD, VS.FAULT_OUTLIER, VS.FAULT_BLIND, VS.FAULT_FRESH, VS.FAULT_RESET) == (1, 2, 4, 8, 16, 32, 64)
    assert len(VS.FAULT_FIELDS) == 15 and len(VS.FAULT_RECORD_FIELDS) == 16 and VS.FAULT_FIELDS.index("max_age") == F.MAX_AGE
    assert VS.FAULT_RECORD_FIELDS.index("chain") == F.CHAIN and VS.FAULT_RECORD_FIELDS.index("longest_gps") == F.LONGEST
    assert np.array_equal(VS.fault_default(), F.NEUTRAL)
    rows = np.full((3, 16), 7.0)
    L = _lib.load()
    assert L.kmpc_sense_faults_default(rows.ctypes.data_as(C.POINTER(C.c_double)), 3) == 0 and (rows == F.NEUTRAL).all()
    assert L.kmpc_sense_faults_default(None, 1) == ARG and b"kmpc_sense_faults_default" in L.kmpc_last_error(None)
    assert L.kmpc_sense_faults_default(None, 0) == 0 and L.kmpc_sense_faults_default(rows.ctypes.data_as(C.POINTER(C.c_double)), -1) == ARG


def test_symbols_are_exported_and_the_abi_version_stays():
    from mkz_mpc_path_follower_amd import _lib
    L = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.kmpc_abi_version() == 8
    assert len(L.kmpc_sense_faults_batch.argtypes) == 17


def test_argument_checks_answer_before_any_device_call():
    from mkz_mpc_path_follower_amd import _lib
    L = _lib.load()
    p = C.c_void_p(64)   # never dereferenced: every call below is refused on the host
    s = dict(B=4, state=p, sensor=p, faults=p, period=0, id_base=0, delay=p, ring=p, depth=3, rec=p, z=p, held=p, flags=p, blind=p)

    def sense(**kw):
        a = dict(s, **kw)
        return L.kmpc_sense_faults_batch(0, a["B"], a["state"], a["sensor"], a["faults"], 1, a["period"], a["id_base"], a["delay"], a["ring"], a["depth"],
                                         a["rec"], a["z"], a["held"], a["flags"], a["blind"], None)
    for bad in (dict(B=-1), dict(period=-1), dict(id_base=-1), dict(state=None), dict(sensor=None), dict(faults=None), dict(rec=None), dict(z=None),
                dict(held=None), dict(delay=None), dict(ring=None), dict(depth=0), dict(depth=-3)):
        assert sense(**bad) == ARG, bad
        assert b"kmpc_sense_faults_batch" in L.kmpc_last_error(None)
    assert sense(B=0) == 0 and sense(B=0, delay=None, ring=None, depth=0) == 0 and sense(B=0, flags=None, blind=None) == 0
    assert sense(B=0, ring=None) == ARG and sense(B=0, depth=0) == ARG


def test_python_validators():
    from mkz_mpc_path_follower_amd import vehicle_sim as VS
    ok = np.tile(F.NEUTRAL, (4, 1))
    assert VS.check_fault_rows(ok) is not None and VS.check_fault_rows(F.committed_case()["faults"]) is not None
    for w, v in ((0, -0.1), (2, 1.5), (3, 2.0), (5, -1.0), (12, 1.01), (6, -1.0), (7, 2.5), (9, 0.5), (11, -3.0), (10, np.inf), (13, -1.0), (13, np.inf),
                 (14, -1.0), (14, -np.inf), (0, np.nan), (9, np.nan), (14, np.nan), (15, np.nan)):
        rows = ok.copy()
        rows[2, w] = v
        with pytest.raises(ValueError):
            VS.check_fault_rows(rows)
    for shape in ((4, 8), (16,)):
        with pytest.raises(ValueError):
            VS.check_fault_rows(np.zeros(shape))
    edge = ok.copy()
    edge[:, 0:6], edge[:, 12], edge[:, 14] = np.array([0, 1, 0.5, 0, 1, 0.5]), 1.0, 0.0
    VS.check_fault_rows(edge)
    with pytest.raises(ValueError):
        VS.fault_params(4, no_such_word=1.0)
    with pytest.raises(ValueError):
        VS.fault_params(4, p_lose=0.1, p_lose_gps=0.2)
    with pytest.raises(ValueError):
        VS.fault_params(4, win_len_gps=np.zeros(5))
    with pytest.raises(ValueError):
        VS.fault_params(4, p_outlier=1.5)


# ---------------------------------------------------------------- one-vehicle CPU loops
@pytest.fixture(scope="module")
def outage_loops(oracle):
    tr, X0, Y0, P0 = F.path3()
    assert len(tr) == 2209
    runs = dict(held=F.cpu_loop(oracle, tr, X0, Y0, P0, F.STEPS, F.window_row(F.WINDOW[1])),
                estimator=F.cpu_loop(oracle, tr, X0, Y0, P0, F.STEPS, F.window_row(F.WINDOW[1]), estimator=True),
                none=F.cpu_loop(oracle, tr, X0, Y0, P0, F.STEPS, F.NEUTRAL, estimator=True))
    return tr, runs


def test_dead_reckoning_beats_the_held_fix(outage_loops):
    """path3 from sample int(0.56 * 2209) on the path at 6 m/s, 150 periods, GPS silent for periods 20 ... 49, no noise.  Largest cross-track
    error of the restatement's loops: held fix 15.68 m, estimator (dead reckoning on heading and speed) 0.83 m, no outage 0.62 m -- the
    prototype's 15.7 / 0.83 / 0.62 m.  (A 100-period window: 58.1 m against 1.13 m.)"""
    tr, runs = outage_loops
    e = {k: F.max_ect(tr, r["state"]) for k, r in runs.items()}
    print("largest cross-track error [m]:", e)
    for r in runs.values():
        assert (r["status"] == 0).all() and not r["latch"].any() and np.isfinite(r["state"]).all()
    assert e["held"] > 5.0 * e["estimator"] and e["estimator"] < e["none"] + 0.5
    h = runs["held"]
    sil = (h["flags"] & 1) == 1
    assert np.array_equal(np.flatnonzero(sil), np.arange(20, 50)) and np.isnan(h["z"][sil, 0:2]).all() and not np.isnan(h["z"][:, 2:]).any()
    assert (h["est"][20:50, 0:2] == h["state"][19, 0:2]).all()                       # the held fix is period 19's
    assert np.array_equal(h["est"][20:50, 2:4], h["state"][20:50, 2:4])              # with a fresh heading and speed
    assert h["fault_record"][F.N_SILENT] == 30 and h["fault_record"][F.LONGEST] == 30 and h["fault_record"][F.AGE] == 0
    assert np.isfinite(runs["estimator"]["seen"]).all()


def test_blind_stop_latches_when_the_age_first_exceeds_the_limit(oracle):
    """MAX_AGE 5, GPS window of 10 from period 20: AGE is 1 in period 20 and first exceeds 5 in period 25; the vehicle latches there, is commanded
    -1.0 / 0.0 from that period on and stays latched after the GPS returns.  Without blind_stop the same run never latches."""
    tr, X0, Y0, P0 = F.path3()
    row = F.window_row(10, w14=5.0)
    r = F.cpu_loop(oracle, tr, X0, Y0, P0, 40, row, estimator=True, blind_stop=True)
    assert np.array_equal(np.flatnonzero(r["blind"]), np.arange(25, 30)) and np.array_equal(np.flatnonzero(r["flags"] & F.F_BLIND), np.arange(25, 30))
    assert np.array_equal(np.flatnonzero(r["latch"]), np.arange(25, 40))
    assert (r["cmd"][25:] == np.array([-1.0, 0.0])).all() and (r["cmd"][:25, 0] != -1.0).all()
    free = F.cpu_loop(oracle, tr, X0, Y0, P0, 40, row, estimator=True)
    assert not free["latch"].any() and np.array_equal(free["blind"], r["blind"]) and np.array_equal(free["cmd"][:25], r["cmd"][:25])
