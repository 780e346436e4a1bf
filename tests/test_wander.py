"""The Gauss-Markov stage on the device: kmpc_wander_batch against the numpy restatement tests/wander_ref.py, its exact properties (off channels,
sharding, A = 1 / Q = 0, neutral rows, containment), and `wander=` in both closed loops.

Tolerances.  An active X at the k-th call from a fresh record lies within (k + 1) * 1e-13 * max(S0_c, Q_c) of the restatement: 1e-13 is the bound on
one normal that tests/test_plant_sensor.py uses for the same library calls (log / sqrt / cos / sin within a few ulp each, |n| < 6.8), every call
adds one more normal scaled by S0 or Q, |A| <= 1 cannot amplify what is there, and the remaining operations are correctly rounded in both.  The
composed words of an active channel follow the same bound; every other word, COUNT, every off channel and everything between two device runs is
compared exactly (torch.equal, or bit patterns where a -0.0 matters).  The loop's `est` against plant_ref.sense: that test's 1e-13 per normal times
the channel's sigma, plus one unit in the last place of the result for the sum the noise is added in.
B = 300 in the kernel tests: one full 256-thread block and a partial one whose last wave is partial too."""
import ctypes as C

import numpy as np
import pytest

import fleet_scenario as F
import plant_ref as R
import road_profile_ref as RP
import wander_ref as W

pytestmark = pytest.mark.gpu

B0 = W.CASE_B
TOL_N = 1e-13


def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64).cuda()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def lib():
    from mkz_mpc_path_follower_amd import _lib
    return _lib.load()


def bits(t):
    """a float64 tensor or array as int64 bit patterns (numpy)"""
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


class Stage:
    """the buffers of one fleet's stage and one call of the entry point; the outputs start as 7.0, so a word nobody wrote shows"""

    def __init__(self, rows, sensor=None, road=None, rec=None):
        import torch
        self.B = len(rows)
        self.rows = dev(rows)
        self.rec = torch.zeros((self.B, 16), dtype=torch.float64, device="cuda") if rec is None else dev(rec)
        self.sensor = None if sensor is None else dev(sensor)
        self.road = None if road is None else dev(road)
        self.sensor_out = None if sensor is None else torch.full((self.B, 8), 7.0, dtype=torch.float64, device="cuda")
        self.road_out = None if road is None else torch.full((self.B, 8), 7.0, dtype=torch.float64, device="cuda")

    def call(self, seed, period, id_base=0):
        assert lib().kmpc_wander_batch(0, self.B, ptr(self.rows), ptr(self.rec), seed, period, id_base, ptr(self.sensor), ptr(self.sensor_out),
                                       ptr(self.road), ptr(self.road_out), None) == 0

    def host(self):
        import torch
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy() for k in ("rec", "sensor_out", "road_out") if getattr(self, k) is not None}


@pytest.fixture(scope="module")
def case():
    return W.mixed_case()


def bound(rows, k):
    """[B,8]: (k + 1) * 1e-13 * max(S0_c, Q_c)"""
    return (k + 1) * TOL_N * np.maximum(rows[:, W.S0:W.S0 + 8], rows[:, W.Q:W.Q + 8])


def check_against_ref(got, ref, rows, k, sensor=None, road=None):
    """one call's outputs against the restatement's -> the largest |difference| / bound over the active words"""
    on = ref["on"]
    bd = bound(rows, k)
    x = got["rec"][:, 0:8]
    assert np.array_equal(got["rec"][:, W.COUNT], ref["rec"][:, W.COUNT])
    assert np.array_equal(bits(x[~on]), np.zeros((~on).sum(), np.int64))                          # off: +0.0
    assert np.array_equal(bits(got["rec"][:, 9:16]), bits(ref["rec"][:, 9:16]))
    d = np.abs(x - ref["x"])
    assert (d[on] <= bd[on]).all(), (k, (d / np.where(bd > 0, bd, 1.0))[on].max())
    worst = (d[on] / bd[on]).max() if on.any() and (bd[on] > 0).all() else 0.0
    if sensor is not None:
        so = got["sensor_out"]
        assert np.array_equal(bits(so[:, 0:4]), bits(sensor[:, 0:4]))
        assert np.array_equal(bits(so[:, 4:8][~on[:, 0:4]]), bits(sensor[:, 4:8][~on[:, 0:4]]))
        ds = np.abs(so[:, 4:8] - ref["sensor_out"][:, 4:8])
        assert (ds[on[:, 0:4]] <= bd[:, 0:4][on[:, 0:4]]).all(), k
    if road is not None:
        ro = got["road_out"]
        assert np.array_equal(bits(ro[:, [0, 1, 5, 6, 7]]), bits(road[:, [0, 1, 5, 6, 7]]))
        for c, w in W.ROAD_WORD.items():
            assert np.array_equal(bits(ro[~on[:, c], w]), bits(road[~on[:, c], w]))
            assert (np.abs(ro[:, w] - ref["road_out"][:, w])[on[:, c]] <= bd[on[:, c], c]).all(), (k, c)
    return worst


# ---------------------------------------------------------------- 1: parity
def test_parity_against_the_restatement(case):
    """the mixed case (stationary, white, constant, walk and off channels scattered over 300 vehicles, id_base 3, a 64-bit seed), 16 periods from a
    fresh record, the restatement fed ITS OWN record call after call.  COUNT exact, an off channel's X +0.0, active X and composed words within
    (k + 1) * 1e-13 * max(S0, Q), every other composed word the base's bits.  Measured on the MI355X: largest |difference| of an active X 4.441e-16, worst |difference| / bound
    4.518e-03 (DESIGN.md section 8a has them)."""
    rows, sensor, road = case["rows"], case["sensor"], case["road"]
    s = Stage(rows, sensor, road)
    rec = np.zeros((B0, 16))
    worst = dx = 0.0
    for k in range(W.CASE_PERIODS):
        s.call(case["seed"], k, 3)
        ref = W.step(rows, rec, case["seed"], k, 3, sensor, road)
        rec = ref["rec"]
        got = s.host()
        worst = max(worst, check_against_ref(got, ref, rows, k, sensor, road))
        dx = max(dx, np.abs(got["rec"][:, 0:8] - ref["x"]).max())
    print("active X against the restatement over 16 periods: worst |difference| / bound = %.3e, largest |difference| %.3e" % (worst, dx))
    assert (got["rec"][:, W.COUNT] == W.CASE_PERIODS).all() and (got["road_out"] != 7.0).all() and (got["sensor_out"] != 7.0).all()


# ---------------------------------------------------------------- 2: counter words
@pytest.mark.parametrize("first,id_base", [(2 ** 33 + 1, 0), (0, 2 ** 32 - 100), (2 ** 61 + 5, 2 ** 40)], ids=["period-hi", "gid-crosses-2^32", "both-hi"])
def test_high_counter_words(case, first, id_base):
    """a fresh record started at period 2^33 + 1 and run for 3 periods; id_base = 2^32 - 100, so gid crosses into the high word inside the batch; and
    both high words at once, the period just below the 2^62 limit's half"""
    rows = case["rows"]
    s = Stage(rows)
    rec = np.zeros((B0, 16))
    for k in range(3):
        s.call(case["seed"], first + k, id_base)
        ref = W.step(rows, rec, case["seed"], first + k, id_base)
        rec = ref["rec"]
        check_against_ref(s.host(), ref, rows, k)
    other = Stage(rows)
    other.call(case["seed"], first + 2 ** 32, id_base)
    on = W.active(rows) & (rows[:, W.S0:W.S0 + 8] > 0)
    first_x = W.step(rows, np.zeros((B0, 16)), case["seed"], first, id_base)["x"]
    assert (other.host()["rec"][:, 0:8][on] != first_x[on]).all()          # the period's high word reaches the generator


# ---------------------------------------------------------------- 3: independence of batch and shard
def test_two_shards_are_one_fleet(case):
    """6 periods: vehicles [0, 77) and [77, 300) as two calls with their id_base equal the slices of the one 300-vehicle call, records and composed
    rows, bit for bit; B = 1 is row 0 of the batch; B = 0 returns 0 without touching anything"""
    import torch
    rows, sensor, road = case["rows"], case["sensor"], case["road"]
    whole = Stage(rows, sensor, road)
    lo, hi = Stage(rows[:77], sensor[:77], road[:77]), Stage(rows[77:], sensor[77:], road[77:])
    one = Stage(rows[:1], sensor[:1], road[:1])
    for p in range(6):
        whole.call(case["seed"], p, 11)
        lo.call(case["seed"], p, 11)
        hi.call(case["seed"], p, 11 + 77)
        one.call(case["seed"], p, 11)
        torch.cuda.synchronize()
        for k in ("rec", "sensor_out", "road_out"):
            assert torch.equal(torch.cat([getattr(lo, k), getattr(hi, k)]), getattr(whole, k)), (p, k)
            assert torch.equal(getattr(one, k), getattr(whole, k)[:1]), (p, k)
    assert (whole.rec[:, 0:8] != 0).any().item()
    before = whole.rec.clone()
    assert lib().kmpc_wander_batch(0, 0, ptr(whole.rows), ptr(whole.rec), 1, 6, 0, None, None, None, None, None) == 0
    assert lib().kmpc_wander_batch(0, 0, None, None, 1, 6, 0, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(whole.rec, before)


# ---------------------------------------------------------------- 4: exact properties
def test_exact_properties(case):
    """A = 1, Q = 0 keeps the first draw: X after 10 periods equals X after the first numerically, and from period 2 on bit for bit (a -0.0 may
    have become +0.0 once).  Neutral rows: both outputs are their bases' bits, every X is +0.0.  Both pairs NULL advance the record identically;
    one pair alone leaves the other consumer's memory unwritten."""
    import torch
    sensor, road = case["sensor"], case["road"]
    const = np.zeros((B0, 24))
    const[:, W.S0:W.S0 + 8], const[:, W.A:W.A + 8] = np.linspace(0.01, 2.0, 8), 1.0
    s = Stage(const, sensor, road)
    xs = []
    for p in range(10):
        s.call(5, p)
        xs.append(s.rec[:, 0:8].clone())
    torch.cuda.synchronize()
    assert (xs[9] == xs[0]).all().item() and (xs[0] != 0).all().item()
    for p in range(2, 10):
        assert np.array_equal(bits(xs[p]), bits(xs[1])), p
    assert torch.equal(s.sensor_out[:, 4:8], s.sensor[:, 4:8] + xs[9][:, 0:4]) and torch.equal(s.road_out[:, 2:5], s.road[:, 2:5] + xs[9][:, 4:7])

    n = Stage(np.tile(W.NEUTRAL, (B0, 1)), sensor, road)
    for p in range(3):
        n.call(5, p)
    g = n.host()
    assert np.array_equal(bits(g["sensor_out"]), bits(sensor)) and np.array_equal(bits(g["road_out"]), bits(road))
    assert not bits(g["rec"][:, 0:8]).any() and (g["rec"][:, W.COUNT] == 3).all() and not g["rec"][:, 9:].any()
    assert np.signbit(road[50:60, 2:5]).all() and np.signbit(g["road_out"][50:60, 2:5]).all()       # a -0.0 base word stays -0.0

    rows = case["rows"]
    # one pair alone: the stage holds all four buffers, but the call is given one pair only -- the other consumer's out keeps its 7.0
    full, bare, half_s, half_r = Stage(rows, sensor, road), Stage(rows), Stage(rows, sensor, road), Stage(rows, sensor, road)
    L = lib()
    for p in range(4):
        full.call(case["seed"], p, 3)
        bare.call(case["seed"], p, 3)
        assert L.kmpc_wander_batch(0, B0, ptr(half_s.rows), ptr(half_s.rec), case["seed"], p, 3, ptr(half_s.sensor), ptr(half_s.sensor_out), None, None, None) == 0
        assert L.kmpc_wander_batch(0, B0, ptr(half_r.rows), ptr(half_r.rec), case["seed"], p, 3, None, None, ptr(half_r.road), ptr(half_r.road_out), None) == 0
    torch.cuda.synchronize()
    for st in (bare, half_s, half_r):
        assert torch.equal(st.rec, full.rec)
    assert torch.equal(half_s.sensor_out, full.sensor_out) and torch.equal(half_r.road_out, full.road_out)
    assert (half_s.road_out == 7.0).all().item() and (half_r.sensor_out == 7.0).all().item()
    assert torch.equal(half_s.road, full.road) and torch.equal(half_r.sensor, full.sensor)


# ---------------------------------------------------------------- 5: containment
def test_a_bad_vehicle_stays_alone(case):
    """8 periods next to a clean run: vehicle 13's row has a NaN (S0 of channel 1), vehicle 25's record gets COUNT = NaN and vehicle 26's COUNT = -1
    before period 4.  Every other vehicle is torch.equal to the clean run in every period; the bad records come out fresh with COUNT == 1 and the
    first-call values of period 4; the NaN stays in vehicle 13's channel 1 and its composed bias_y"""
    import torch
    rows, sensor, road = case["rows"], case["sensor"], case["road"]
    bad_rows = rows.copy()
    bad_rows[13, W.S0 + 1] = np.nan
    clean, dirty = Stage(rows, sensor, road), Stage(bad_rows, sensor, road)
    keep = torch.ones(B0, dtype=torch.bool, device="cuda")
    keep[[13, 25, 26]] = False
    fresh4 = Stage(rows, sensor, road)
    fresh4.call(case["seed"], 4, 3)
    for p in range(8):
        if p == 4:
            dirty.rec[25, W.COUNT], dirty.rec[26, W.COUNT] = float("nan"), -1.0
        clean.call(case["seed"], p, 3)
        dirty.call(case["seed"], p, 3)
        torch.cuda.synchronize()
        for k in ("rec", "sensor_out", "road_out"):
            assert torch.equal(getattr(clean, k)[keep], getattr(dirty, k)[keep]), (p, k)
        assert torch.isnan(dirty.rec[13, 1]).item() and torch.isnan(dirty.sensor_out[13, 5]).item()
        other = [c for c in range(8) if c != 1]
        assert torch.equal(dirty.rec[13, other], clean.rec[13, other]) and dirty.rec[13, W.COUNT].item() == p + 1
        if p == 4:
            assert (dirty.rec[25:27, W.COUNT] == 1).all().item() and torch.equal(dirty.rec[25:27], fresh4.rec[25:27])
            assert torch.equal(dirty.sensor_out[25:27], fresh4.sensor_out[25:27]) and torch.equal(dirty.road_out[25:27], fresh4.road_out[25:27])
    assert (dirty.rec[25:27, W.COUNT] == 4).all().item() and (clean.rec[:, W.COUNT] == 8).all().item()


# ---------------------------------------------------------------- 6: the loops
LB, LN, LSTEPS, LVT = 64, 8, 12, 6.0


def fleet_starts():
    """64 vehicles on the three fixture paths, vehicle b on path b % 3, on the path between 5 % and 55 % of its length -> (path ids, X0, Y0, Psi0)"""
    pid = np.arange(LB) % 3
    X0, Y0, P0 = np.zeros(LB), np.zeros(LB), np.zeros(LB)
    for b in range(LB):
        tr = F.trajectory(int(pid[b]))
        i = int((0.05 + 0.5 * (b // 3) / 21.0) * len(tr))
        X0[b], Y0[b], P0[b] = tr[i, 4], tr[i, 5], tr[i, 3]
    return pid, X0, Y0, P0


def make_loop(kind, wander_rows=None, sensor=True, road=None, profile_table=None, seed=21, **sensor_kw):
    """a 64-vehicle loop at 6 m/s; wander_rows: [64,24] or None (no wander=); road: dict of road_params overrides or None (no road=)"""
    import torch
    from mkz_mpc_path_follower_amd import FleetRefTrajectory
    from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop, ClosedLoopFrenet
    from mkz_mpc_path_follower_amd.vehicle_sim import RoadProfile, SensorModel, VehicleSimulator, Wander, road_params
    pid, X0, Y0, P0 = fleet_starts()
    grt = FleetRefTrajectory([F.path_dict(p) for p in range(3)], pid.tolist(), time_mode=[0] * LB, traj_horizon=LN, traj_dt=0.2)
    kw = {}
    if road is not None:
        kw["road"] = road_params(LB, **road)
    if profile_table is not None:
        kw["road_profile"] = RoadProfile(grt, profile_table)
    sim = VehicleSimulator(LB, X0=X0, Y0=Y0, Psi0=P0, **kw)
    sim.state[:, 3] = LVT
    lkw = {}
    if sensor:
        lkw["sensor"] = SensorModel(LB, seed=3, **sensor_kw)
    if wander_rows is not None:
        lkw["wander"] = Wander(LB, wander_rows, seed=seed)
    if kind == "frenet":
        return ClosedLoopFrenet(grt, sim, LN, LVT, **lkw)
    return ClosedLoop(grt, sim, N=LN, target_vel=LVT, **lkw)


KINDS = ["cartesian", "frenet"]


@pytest.mark.parametrize("kind", KINDS)
def test_neutral_wander_leaves_the_loops_bit_for_bit(kind):
    """sensor (noise and bias) and road (bank, offset) present, wander= of neutral rows: state, cmd and status histories torch.equal to the loop
    without wander=; the caller's rows have moved to params_base / road_base and the rows read equal them; without wander= nothing is new"""
    import torch
    skw = dict(sigma=(0.05, 0.05, 0.005, 0.05), bias=(0.1, -0.1, 0.01, 0.0))
    road = dict(mu=0.9, a_lat=0.4, df_offset=0.002)
    plain = make_loop(kind, None, road=road, **skw)
    a = plain.run(LSTEPS, history=True)
    loop = make_loop(kind, np.tile(W.NEUTRAL, (LB, 1)), road=road, **skw)
    b = loop.run(LSTEPS, history=True)
    torch.cuda.synchronize()
    for k in ("state", "cmd", "status", "est"):
        assert torch.equal(a[k], b[k]), k
    assert "wander" not in a and tuple(b["wander"].shape) == (LSTEPS, LB, 8) and not bits(b["wander"]).any()
    assert plain.wander is None and plain.sensor.params_base is None and plain.sim.road_base is None and plain.sim.road_mid is None
    s, sim = loop.sensor, loop.sim
    assert s.params_base is not None and s.params.data_ptr() != s.params_base.data_ptr() and torch.equal(s.params, s.params_base)
    assert sim.road.data_ptr() != sim.road_base.data_ptr() and torch.equal(sim.road, sim.road_base)
    assert (loop.wander.rec[:, W.COUNT] == LSTEPS).all().item() and (b["state"][LSTEPS, :, 3] > 1.0).all().item()
    assert not torch.equal(b["est"], b["state"][:LSTEPS, :, 0:4])


@pytest.mark.parametrize("kind", KINDS)
def test_constant_wander_is_a_preset_road(kind):
    """loop one: A_LAT and DF_OFFSET channels at A = 1, Q = 0 (a random constant per vehicle) on neutral road rows; loop two: no wander, road rows
    preset to the X the first call drew (0 + X is X).  `state` is torch.equal over all periods: the composition reaches the plant exactly"""
    import torch
    from mkz_mpc_path_follower_amd.vehicle_sim import Wander
    rows = np.zeros((LB, 24))
    rows[:, W.S0 + W.CH_A_LAT], rows[:, W.S0 + W.CH_DF_OFFSET] = 0.8, 0.01
    rows[:, W.A + W.CH_A_LAT], rows[:, W.A + W.CH_DF_OFFSET] = 1.0, 1.0
    one = make_loop(kind, rows, sensor=False, road={})
    a = one.run(LSTEPS, history=True)
    alone = Wander(LB, rows, seed=21)
    x = alone.step(0).cpu().numpy()
    assert (x[:, [5, 6]] != 0).all() and (x[:, [0, 1, 2, 3, 4, 7]] == 0).all()
    two = make_loop(kind, None, sensor=False, road=dict(a_lat=x[:, 5], df_offset=x[:, 6]))
    b = two.run(LSTEPS, history=True)
    torch.cuda.synchronize()
    assert torch.equal(a["state"], b["state"]) and torch.equal(a["cmd"], b["cmd"])
    assert (a["wander"] == a["wander"][0]).all().item() and torch.equal(one.sim.road, two.sim.road)
    flat = make_loop(kind, None, sensor=False, road={}).run(LSTEPS, history=True)
    assert not torch.equal(flat["state"], a["state"])                       # the gust does reach the plant


@pytest.mark.parametrize("kind", KINDS)
def test_gust_and_coloured_gps_together(kind):
    """coloured GPS error (x, y: sigma 0.3 m, tau 5 s), a heading walk, a lateral gust (sigma 0.5 m/s^2, tau 1 s) and the free channel, with a white
    sensor on top: hist["wander"] is a stand-alone Wander stepped with the same seed (torch.equal); hist["est"] is plant_ref.sense of hist["state"]
    under the composed bias, within 1e-13 * sigma per channel + one unit in the last place of the result"""
    import torch
    from mkz_mpc_path_follower_amd.vehicle_sim import Wander, wander_rows
    rows = wander_rows(LB, sigma=(0.3, 0.3, 0, 0, 0, 0.5, 0, 1.0), tau=(5.0, 5.0, 0, 0, 0, 1.0, 0, 2.0), walk=(0, 0, 0.002, 0, 0, 0, 0, 0))
    sigma, bias = np.array([0.05, 0.05, 0.005, 0.05]), np.array([0.1, -0.1, 0.01, 0.0])
    loop = make_loop(kind, rows, road=dict(mu=1.0), sigma=tuple(sigma), bias=tuple(bias))
    h = loop.run(LSTEPS, history=True)
    alone = Wander(LB, rows, seed=21)
    xs = torch.stack([alone.step(k).clone() for k in range(LSTEPS)])
    torch.cuda.synchronize()
    assert torch.equal(h["wander"], xs) and (h["wander"][1:, :, [0, 1, 2, 5, 7]] != 0).all().item() and not bits(h["wander"][:, :, [3, 4, 6]]).any()
    assert torch.equal(loop.sim.road[:, 3], loop.sim.road_base[:, 3] + xs[-1][:, 5]) and torch.equal(loop.sim.road[:, [0, 1, 2, 4, 5, 6, 7]], loop.sim.road_base[:, [0, 1, 2, 4, 5, 6, 7]])
    state, est, x = h["state"].cpu().numpy(), h["est"].cpu().numpy(), xs.cpu().numpy()
    worst = 0.0
    for k in range(LSTEPS):
        srow = np.tile(np.concatenate([sigma, bias]), (LB, 1))
        srow[:, 4:7] = srow[:, 4:7] + x[k][:, 0:3]                          # channel 3 is off: bias_v keeps its bits
        want = R.sense(state[k], srow, 3, k)
        tol = TOL_N * sigma + np.spacing(np.abs(want))
        d = np.abs(est[k] - want)
        assert (d <= tol).all(), (k, (d / tol).max())
        worst = max(worst, (d / tol).max())
    print("est against plant_ref.sense under the composed bias: worst |difference| / tolerance = %.3e" % worst)
    assert torch.equal(loop.sensor.params[:, 4:7], loop.sensor.params_base[:, 4:7] + xs[-1][:, 0:3])
    assert torch.equal(loop.sensor.params[:, [0, 1, 2, 3, 7]], loop.sensor.params_base[:, [0, 1, 2, 3, 7]])


def test_the_wander_acts_before_the_road_profile():
    """a truth table with random grip scale, grade and bank per sample, base rows with grip and bank, wander on a_long, a_lat, df_offset: sim.road
    after one period is road_profile_ref.compose of the rows (base + X) at the state the period began in, bit for bit; sim.road_mid is (base + X)"""
    import torch
    trajs = [F.trajectory(p) for p in range(3)]
    rng = np.random.default_rng(77)
    tab = RP.table(trajs)
    for t in tab:
        t[:, 0], t[:, 1], t[:, 2] = rng.uniform(0.5, 1.0, len(t)), rng.normal(0, 0.3, len(t)), rng.normal(0, 0.5, len(t))
    rows = np.zeros((LB, 24))
    rows[:, W.S0 + 4:W.S0 + 7], rows[:, W.A + 4:W.A + 7] = (0.3, 0.6, 0.01), 0.9
    rows[:, W.Q + 4:W.Q + 7] = rows[:, W.S0 + 4:W.S0 + 7] * np.sqrt(1 - 0.81)
    loop = make_loop("cartesian", rows, sensor=False, road=dict(mu=0.9, a_lat=0.2, a_long=-0.1), profile_table=RP.flat(tab))
    for steps in (1, 2):
        h = loop.run(1, history=True)
        torch.cuda.synchronize()
        base, x, st = loop.sim.road_base.cpu().numpy(), h["wander"][0].cpu().numpy(), h["state"][0].cpu().numpy()
        mid = base.copy()
        mid[:, 2:5] = base[:, 2:5] + x[:, 4:7]
        want, closest = RP.compose(trajs, tab, np.arange(LB) % 3, st[:, 0], st[:, 1], mid)
        assert (closest >= 0).all() and np.array_equal(bits(loop.sim.road_mid), bits(mid)) and np.array_equal(bits(loop.sim.road), bits(want)), steps
        assert (want[:, 3] != mid[:, 3]).all() and (mid[:, 3] != base[:, 3]).all() and (want[:, 0] < base[:, 0]).all()


def test_constructor_refusals():
    from mkz_mpc_path_follower_amd.vehicle_sim import SensorModel, Wander
    sens, road, free = np.zeros((LB, 24)), np.zeros((LB, 24)), np.zeros((LB, 24))
    sens[:, W.S0 + 1], road[:, W.Q + 6], free[:, W.S0 + 7] = 0.1, 0.01, 1.0
    with pytest.raises(ValueError):
        make_loop("cartesian", sens, sensor=False, road={})                 # active measurement channels without sensor=
    with pytest.raises(ValueError):
        make_loop("frenet", road, sensor=True)                              # active road channels without road=
    loop = make_loop("cartesian", free, sensor=False)                       # the free channel needs nobody
    assert loop._wander_rows == (None, None, None, None)
    for bad in (Wander(LB + 1, np.zeros((LB + 1, 24))), Wander(LB, free, device="cpu"), "wander"):
        with pytest.raises(ValueError):
            type(loop)(loop.grt, loop.sim, N=LN, target_vel=LVT, wander=bad)
    with pytest.raises(ValueError):
        type(loop)(loop.grt, loop.sim, N=LN, target_vel=LVT, sensor=SensorModel(LB), wander=Wander(LB, road))
