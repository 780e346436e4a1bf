"""CPU side of the road row (kmpc_road_default, kmpc_sim_advance_road): the symbols and their argument checks (no GPU needed: every check comes
before the first device call), the numpy restatement tests/road_ref.py against the queue's restatement and against known answers, the host
validation of road_params / check_road_rows / VehicleSimulator(road=), and the CPU closed loop through a corner with less grip than it asks for."""
import ctypes as C

import numpy as np
import pytest

import latency_ref as LR
import plant_ref as R
import road_ref as RR

ARG = -1   # KMPC_ERR_ARG
MUS = (1.0, 0.7, 0.5, 0.35, 0.25)


def test_symbols_default_row_and_abi_version():
    from mkz_mpc_path_follower_amd import _lib
    from mkz_mpc_path_follower_amd import vehicle_sim as VS
    L = _lib.load()
    for name in ("kmpc_road_default", "kmpc_sim_advance_road"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.kmpc_abi_version() == 8
    row = np.full(8, 7.0)
    assert L.kmpc_road_default(row.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert row.tolist() == [np.inf, np.inf, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0] and np.array_equal(row, RR.NEUTRAL_ROW)
    assert L.kmpc_road_default(None) == ARG and b"kmpc_road_default" in L.kmpc_last_error(None)
    assert np.array_equal(VS.road_default(), row) and VS.ROAD_FIELDS == RR.FIELDS


def test_argument_checks_answer_before_any_device_call():
    from mkz_mpc_path_follower_amd import _lib
    L = _lib.load()
    p = C.c_void_p(64)   # never dereferenced: every call below is refused on the host
    q = dict(B=2, state=p, cmd=p, plant=p, road=p, delay=p, queue=p, depth=4, period=0, n=10, stat=p)

    def road(**kw):
        a = dict(q, **kw)
        return L.kmpc_sim_advance_road(0, a["B"], a["state"], a["cmd"], a["plant"], a["road"], a["delay"], a["queue"], a["depth"], a["period"], a["n"],
                                       a["stat"], None)
    for bad in (dict(road=None), dict(B=-1), dict(n=-1), dict(state=None), dict(cmd=None), dict(plant=None), dict(depth=1), dict(depth=0),
                dict(period=-1), dict(queue=None), dict(road=None, stat=None)):
        assert road(**bad) == ARG, bad
        assert b"kmpc_sim_advance_road" in L.kmpc_last_error(None)
    assert road(B=0) == 0 and road(n=0) == 0 and road(B=0, road=None, stat=None) == 0      # nothing to do: success without a launch
    assert road(B=0, queue=None) == ARG and road(n=0, depth=1) == ARG                      # ... but the queue's own checks still hold
    assert road(n=0, road=None) == ARG


@pytest.mark.parametrize("n", [10, 7])
def test_neutral_rows_restate_the_queue_bit_for_bit(n):
    """300 vehicles with +-30 % plant rows, 6 periods, depth 4, delays 0 ... 30: road_ref with neutral rows is latency_ref.advance_queue, and the
    statistics stay zero"""
    depth, periods = 4, 6
    s0, _, plant = R.spread_case()
    B = len(s0)
    rng = np.random.default_rng(200 + n)
    delay = rng.integers(0, 31, B)
    cmds = np.stack([rng.uniform(-1, 1, (periods, B)), rng.uniform(-0.5, 0.5, (periods, B))], 2)
    road = RR.rows(B)
    a, b, stat = s0, s0, np.zeros((B, 4))
    for p in range(periods):
        a, stat = RR.advance_road(a, cmds, p, plant, road, delay, depth, n, stat=stat)
        b = LR.advance_queue(b, cmds, p, plant, delay, depth, n)
        assert np.array_equal(a, b), (n, p)
    assert not stat.any() and np.isfinite(a).all()


def test_grade_is_a_constant_specific_force():
    """straight ahead at 10 m/s, zero command: after 100 updates (1 s) vx = 10 + A_LONG within 1e-11 (a thousand additions at ulp(10) bound it near
    2e-12), Y, vy and wz exactly 0"""
    a_long = np.array([-0.5, 0.5, -2.0])
    s0 = np.zeros((3, 8))
    s0[:, 3] = 10.0
    s, stat = RR.update_road(s0, np.zeros((3, 2)), np.tile(R.DEFAULT_ROW, (3, 1)), RR.rows(3, a_long=a_long), n_updates=100)
    err = np.abs(s[:, 3] - (10.0 + a_long * 1.0))
    print("grade: |vx - (10 + A_LONG)| =", err)
    assert (err <= 1e-11).all()
    assert not s[:, 1].any() and not s[:, 4].any() and not s[:, 5].any() and not stat.any()


def step_steer(mu, periods=30):
    """0.2 rad commanded at 15 m/s, default plant, one vehicle per mu -> (state, stat) after `periods` periods of 10 updates"""
    B = len(mu)
    s = np.zeros((B, 8))
    s[:, 3] = 15.0
    cmd = np.tile([0.0, 0.2], (B, 1))
    stat = np.zeros((B, 4))
    for _ in range(periods):
        s, stat = RR.update_road(s, cmd, np.tile(R.DEFAULT_ROW, (B, 1)), RR.rows(B, mu=np.asarray(mu, dtype=np.float64)), n_updates=10, stat=stat)
    return s, stat


def test_step_steer_runs_out_of_grip_in_order():
    """mu = 1.0 never saturates and equals mu = inf bit for bit; over mu = 1.0 ... 0.25 the final yaw rate falls strictly and the saturated sub-steps
    rise strictly from 0.  This restatement: final wz 0.514, 0.418, 0.346, 0.250, 0.179 rad/s at peak utilisation 0.79 for mu = 1.0 (printed below)."""
    s, stat = step_steer((np.inf,) + MUS)
    print("step steer: wz", s[:, 5], "saturated front", stat[:, 0], "rear", stat[:, 1], "utilisation", stat[:, 2], stat[:, 3])
    assert np.array_equal(s[0], s[1]) and stat[1, 0] == 0 and stat[1, 1] == 0 and 0.5 < stat[1, 2:4].max() < 1.0
    assert stat[0, 2] == 0.0 and stat[0, 3] == 0.0                     # an infinite limit: utilisation 0 by the division itself
    wz, sat = s[1:, 5], stat[1:, 0] + stat[1:, 1]
    assert (np.diff(wz) < 0).all() and wz[-1] > 0
    assert sat[0] == 0 and (np.diff(sat) > 0).all()
    assert (stat[2:, 2:4].max(1) > 1.0).all()


def test_clip_keeps_bits_and_passes_nan():
    x = np.array([0.3, -0.3, 5.0, -5.0, np.nan, -0.0, 2.0])
    lim = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, np.inf])
    out = RR.clip(x, lim)
    assert np.array_equal(out[:4], [0.3, -0.3, 1.0, -1.0]) and np.isnan(out[4]) and np.signbit(out[5]) and out[6] == 2.0


def test_random_rows_seed_keeps_the_count_comparison_meaningful():
    """the GPU test compares saturation counts exactly except for vehicles whose restated |F| / lim came within 1e-9 of 1 in some sub-step: with the
    committed seed those are at most 1 % of the 300, and the case does saturate"""
    s0, cmd, plant = R.spread_case()
    road = RR.random_rows()
    assert np.isinf(road[:, 0]).sum() > 100 and np.isfinite(road[:, 0]).sum() > 100 and (road[:, 0:2] >= 0.2).all()
    near = np.zeros(len(s0), dtype=bool)
    s, stat = RR.update_road(s0, cmd, plant, road, n_updates=10, near=near)
    print("random rows: vehicles near a limit %d, saturated front %d rear %d" % (near.sum(), (stat[:, 0] > 0).sum(), (stat[:, 1] > 0).sum()))
    assert near.mean() <= 0.01
    assert (stat[:, 0] > 0).sum() >= 10 and (stat[:, 1] > 0).sum() >= 10 and np.isfinite(s).all()
    assert not stat[np.isinf(road[:, 0]), 0].any() and not stat[np.isinf(road[:, 0]), 2].any()


def test_host_validation_without_a_gpu():
    import torch
    from mkz_mpc_path_follower_amd import vehicle_sim as VS
    r = VS.road_params(3, device="cpu")
    assert r.dtype == torch.float64 and tuple(r.shape) == (3, 8) and np.array_equal(r.numpy(), RR.rows(3))
    r = VS.road_params(3, device="cpu", mu=0.5, a_lat=[0.0, 0.75, 1.5], df_offset=0.03, a_long=-0.5, acc_gain=0.9)
    assert np.array_equal(r.numpy(), RR.rows(3, mu=0.5, a_lat=[0.0, 0.75, 1.5], df_offset=0.03, a_long=-0.5, acc_gain=0.9))
    r = VS.road_params(3, device="cpu", mu_f=[0.3, np.inf, 1.0], mu_r=0.8)
    assert r[:, 0].tolist() == [0.3, np.inf, 1.0] and r[:, 1].tolist() == [0.8] * 3
    nan, inf = float("nan"), float("inf")
    for bad in (dict(mu=nan), dict(mu_f=0.0), dict(mu_r=-0.2), dict(mu=-inf), dict(a_long=nan), dict(a_long=inf), dict(a_lat=-inf), dict(df_offset=inf),
                dict(df_offset=[0.0, nan, 0.0]), dict(acc_gain=0.0), dict(acc_gain=-1.0), dict(acc_gain=inf), dict(acc_gain=nan), dict(mu=[0.5, 0.5]),
                dict(mu=[[0.5, 0.5, 0.5]]), dict(grip=0.5), dict(mu=0.5, mu_f=0.4)):
        with pytest.raises(ValueError):
            VS.road_params(3, device="cpu", **bad)
    good = RR.rows(3, mu=0.5)
    assert VS.check_road_rows(good) is not None
    for w, v in ((0, nan), (1, 0.0), (0, -1.0), (2, inf), (3, nan), (4, -inf), (5, 0.0), (5, inf), (6, nan), (7, inf)):
        rows = good.copy()
        rows[1, w] = v
        with pytest.raises(ValueError):
            VS.check_road_rows(rows)
        with pytest.raises(ValueError):
            VS.VehicleSimulator(3, road=rows)                      # refused before the GPU is touched
    for shape in ((8,), (3, 4), (2, 3, 8)):
        with pytest.raises(ValueError):
            VS.check_road_rows(np.ones(shape))
    for rows in (RR.rows(2), RR.rows(3)[:, :6], torch.ones((4, 8), dtype=torch.float64)):
        with pytest.raises(ValueError):
            VS.VehicleSimulator(3, road=rows)
    with pytest.raises(ValueError):
        VS.VehicleSimulator(3, road=good, cmd_queue_depth=1)


def test_cpu_loop_through_a_corner_with_less_grip_than_it_asks_for():
    """path3 at 58 %, already at 6 m/s, 120 periods, the oracle's condensed solver warm-started, no stop latch; vehicles: neutral, mu = 0.5, mu = 0.35.
    Every solve is Optimal; the neutral vehicle never saturates and mu = 0.5 does; mu = 0.5 stays within 0.2 m of the neutral vehicle's largest
    cross-track error and mu = 0.35 leaves with more than twice it.
    This restatement's figures (rms e_ct, max |e_ct| [m], front saturated sub-steps) are printed below and recorded in profiles/README.md's entry of
    the road sweep; the issue's prototype gave 0.221 / 0.621 / 0, 0.243 / 0.701 / 890 and 1.277 / 3.288 / 3676."""
    from oracle import oracle as O
    runs, _tr = RR.cpu_loops(O)
    out = []
    for ri in range(3):
        r = runs[(ri, 0.0)]
        out.append((float(np.sqrt((r["ect"] ** 2).mean())), float(r["ect"].max()), int(r["stat"][0]), int((r["status"] != 0).sum())))
        print("cpu loop %-12s rms e_ct %.3f m, max |e_ct| %.3f m, front saturated %d, rear %d, not Optimal %d"
              % (RR.LOOP_ROADS[ri] or "neutral", out[-1][0], out[-1][1], out[-1][2], int(r["stat"][1]), out[-1][3]))
        assert np.isfinite(r["state"]).all()
    assert all(o[3] == 0 for o in out)
    assert out[0][2] == 0 and out[1][2] > 0
    assert abs(out[1][1] - out[0][1]) <= 0.2
    assert out[2][1] > 2.0 * out[0][1]
