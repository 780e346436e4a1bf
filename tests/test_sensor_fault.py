"""Sensor faults on the device: kmpc_sense_faults_batch against the measurement kernels it extends (bit for bit), against the numpy restatement
of tests/sensor_fault_ref.py (exact: what the stage adds is selections and integer counts), and the loops' `faults=` / `blind_stop=` against the
plain sensor and against the one-vehicle CPU loops of tests/test_sensor_fault_ref.py.

Tolerances.  Tests 1-5 and 7 are exact (torch.equal / array_equal).  Test 6, the device loop against the CPU loop: the project's rule, 10 x the
difference measured on the MI355X, capped at 1e-6 m.  Measured: MEASURED_LOOP below.
B = 300 in the kernel tests: two 256-thread blocks, the second partial."""
import ctypes as C

import numpy as np
import pytest

import latency_ref as LR
import sensor_fault_ref as F

pytestmark = pytest.mark.gpu

B0 = F.CASE_B
# measured on the MI355X: 4 vehicles x 2 loops (held fix, estimator), 80 periods on path3, against sensor_fault_ref.cpu_loop -- largest position
# difference [m]; largest difference of the other states and the commands; of the held state, the estimate and the finite words of z -- see
# test_loop_matches_the_cpu_loops' docstring; bound = 10 x, capped at 1e-6
MEASURED_LOOP = (2.058e-11, 1.072e-10, 2.425e-11)      # the held-fix loop's; the estimator loop's are 1.255e-11, 7.523e-11, 1.704e-11
TOL_LOOP = np.array([2.1e-10, 1.1e-9, 2.5e-10])


def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64).cuda()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def lib():
    from mkz_mpc_path_follower_amd import _lib
    return _lib.load()


class Stage:
    """the buffers of one fleet's fault stage and one call of the entry point"""

    def __init__(self, B, faults, delay=None, depth=0):
        import torch
        self.B, self.faults, self.depth = B, dev(faults), depth
        self.rec = torch.zeros((B, 16), dtype=torch.float64, device="cuda")
        self.z = torch.full((B, 4), 7.0, dtype=torch.float64, device="cuda")
        self.held = torch.full((B, 4), 7.0, dtype=torch.float64, device="cuda")
        self.flags = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        self.blind = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
        self.delay = None if delay is None else dev(delay, torch.int32)
        self.ring = None if delay is None else torch.full((depth, B, 4), float("nan"), dtype=torch.float64, device="cuda")

    def call(self, state, sensor, seed, period, id_base):
        assert lib().kmpc_sense_faults_batch(0, self.B, ptr(state), ptr(sensor), ptr(self.faults), seed, period, id_base, ptr(self.delay), ptr(self.ring),
                                             self.depth, ptr(self.rec), ptr(self.z), ptr(self.held), ptr(self.flags), ptr(self.blind), None) == 0

    def host(self):
        import torch
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy() for k in ("rec", "z", "held", "flags", "blind")}


def plain(state, sensor, seed, period, id_base):
    import torch
    est = torch.empty((state.shape[0], 4), dtype=torch.float64, device="cuda")
    assert lib().kmpc_sense_batch(0, state.shape[0], ptr(state), ptr(sensor), seed, period, id_base, ptr(est), None) == 0
    return est


@pytest.fixture(scope="module")
def case():
    c = F.committed_case()
    c["states_d"] = [dev(s) for s in c["states"]]
    c["sensor_d"] = dev(c["sensor"])
    return c


@pytest.fixture(scope="module")
def case_ref(case):
    return F.run_case(case)


# ---------------------------------------------------------------- 1: neutral rows
def test_neutral_rows_are_the_plain_kernels(case):
    """6 periods of the committed case's states with the neutral row in every vehicle: z and held are kmpc_sense_batch's est, and with a ring
    (ages 0, 1, 2, 9, -1, depth 3, the ring starting as NaN) kmpc_sense_delayed_batch's est and ring; the flags show FRESH in the first call only"""
    import torch
    L = lib()
    neutral = np.tile(F.NEUTRAL, (B0, 1))
    lat = np.random.default_rng(3).permutation(np.resize(np.array((0, 1, 2, 9, -1)), B0))
    a, b = Stage(B0, neutral), Stage(B0, neutral, delay=lat, depth=3)
    ring = torch.full((3, B0, 4), float("nan"), dtype=torch.float64, device="cuda")
    est = torch.empty((B0, 4), dtype=torch.float64, device="cuda")
    for p in range(6):
        st = case["states_d"][p]
        a.call(st, case["sensor_d"], case["seed"], p, case["id_base"])
        b.call(st, case["sensor_d"], case["seed"], p, case["id_base"])
        want = plain(st, case["sensor_d"], case["seed"], p, case["id_base"])
        assert L.kmpc_sense_delayed_batch(0, B0, ptr(st), ptr(case["sensor_d"]), case["seed"], p, case["id_base"], ptr(b.delay), ptr(ring), 3, ptr(est), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(a.z, want) and torch.equal(a.held, want), p
        assert torch.equal(b.z, est) and torch.equal(b.held, est), p
        assert torch.equal(b.ring[p % 3], ring[p % 3]) and torch.equal(b.ring[p % 3], st[:, 0:4])
        for s in (a, b):
            assert (s.flags == (F.F_FRESH if p == 0 else 0)).all().item() and not s.blind.any().item()
            assert (s.rec[:, F.COUNT] == p + 1).all().item() and (s.rec[:, F.CHAIN:] == 0).all().item() and torch.equal(s.rec[:, 0:4], s.held)
    assert not torch.equal(b.z, a.z) and not torch.isnan(b.ring).any().item()


# ---------------------------------------------------------------- 2: the committed case
def test_committed_case_matches_the_restatement_exactly(case, case_ref):
    """40 periods: the NaN pattern, flags, blind and the record's COUNT / CHAIN / AGE / counters equal the restatement's (selections and integer
    counts); every delivered value equals kmpc_sense_batch run on the device with that period's effective sigma row (an outlier's SIGMA_X, SIGMA_Y
    replaced); held values equal the restatement's selection applied to those device values"""
    import torch
    s = Stage(B0, case["faults"])
    last = np.zeros((B0, 4))
    for p in range(F.CASE_PERIODS):
        s.call(case["states_d"][p], case["sensor_d"], case["seed"], p, case["id_base"])
        m = plain(case["states_d"][p], dev(case_ref["sensor_eff"][p]), case["seed"], p, case["id_base"])
        g = s.host()
        m = m.cpu().numpy()
        sil_c = case_ref["silent"][p][:, F.SOURCE_OF]
        assert np.array_equal(np.isnan(g["z"]), sil_c), p
        assert np.array_equal(g["flags"], case_ref["flags"][p]) and np.array_equal(g["blind"], case_ref["blind"][p]), p
        assert np.array_equal(g["rec"][:, F.COUNT:], case_ref["rec"][p][:, F.COUNT:]), p
        assert np.array_equal(g["z"][~sil_c], m[~sil_c]), p
        last = np.where(sil_c, last, m)
        assert np.array_equal(g["held"], last) and np.array_equal(g["rec"][:, 0:4], last), p
    assert np.isnan(g["z"]).any() and (g["rec"][:, F.N_OUTLIER] > 0).sum() >= 80 and (g["rec"][:, F.LONGEST:F.LONGEST + 3] > 5).any()


# ---------------------------------------------------------------- 3: sharding
def test_two_shards_are_one_fleet(case):
    """12 periods: one call of 300 equals a call of 130 and a call of 170 with id_base moved on, bit for bit, records included"""
    import torch
    whole = Stage(B0, case["faults"])
    lo, hi = Stage(130, case["faults"][:130]), Stage(170, case["faults"][130:])
    for p in range(12):
        st, sr = case["states_d"][p], case["sensor_d"]
        whole.call(st, sr, case["seed"], p, case["id_base"])
        lo.call(st[:130].contiguous(), sr[:130].contiguous(), case["seed"], p, case["id_base"])
        hi.call(st[130:].contiguous(), sr[130:].contiguous(), case["seed"], p, case["id_base"] + 130)
        torch.cuda.synchronize()
        for k in ("rec", "z", "held", "flags", "blind"):
            both = torch.cat([getattr(lo, k), getattr(hi, k)])
            w = getattr(whole, k)
            assert torch.equal(torch.nan_to_num(both, nan=-12345.0), torch.nan_to_num(w, nan=-12345.0)) if w.is_floating_point() else torch.equal(both, w), (p, k)
    assert torch.isnan(whole.z).any().item()


# ---------------------------------------------------------------- 4: containment
def test_a_bad_vehicle_stays_alone(case):
    """10 periods next to a clean run: vehicle 13 (chains) has an all-NaN row, vehicle 25 (chains)'s record is poisoned before period 4 (COUNT = NaN) and
    vehicle 26 (windows)'s before period 6 (CHAIN = 9), vehicle 40 (everything)'s truth is non-finite throughout.  Every other vehicle's outputs and records
    are the clean run's in every period; the poisoned records come back fresh with RESET; the NaN row does nothing (a NaN compares false)."""
    import torch
    bad_rows = case["faults"].copy()
    bad_rows[13] = np.nan
    clean, dirty = Stage(B0, case["faults"]), Stage(B0, bad_rows)
    keep = np.ones(B0, bool)
    keep[[13, 25, 26, 40]] = False
    for p in range(10):
        st = case["states_d"][p]
        bad_st = st.clone()
        bad_st[40, 0:4] = torch.tensor([float("nan"), float("inf"), float("-inf"), float("nan")], dtype=torch.float64)
        if p == 4:
            dirty.rec[25, F.COUNT] = float("nan")
        if p == 6:
            dirty.rec[26, F.CHAIN] = 9.0
        clean.call(st, case["sensor_d"], case["seed"], p, case["id_base"])
        dirty.call(bad_st, case["sensor_d"], case["seed"], p, case["id_base"])
        c, d = clean.host(), dirty.host()
        for k in c:
            assert np.array_equal(c[k][keep], d[k][keep], equal_nan=True), (p, k)
        assert d["flags"][13] == (F.F_FRESH if p == 0 else 0) and not np.isnan(d["z"][13]).any()
        if p == 4:
            assert d["flags"][25] == F.F_FRESH | F.F_RESET and d["rec"][25, F.COUNT] == 1 and (d["rec"][25, F.CHAIN:] == 0).all() and not np.isnan(d["z"][25]).any()
        if p == 6:
            assert d["flags"][26] == F.F_FRESH | F.F_RESET and d["rec"][26, F.COUNT] == 1 and (d["rec"][26, F.CHAIN:] == 0).all()
        assert np.array_equal(d["flags"][40], c["flags"][40]) and np.array_equal(d["rec"][40, F.COUNT:], c["rec"][40, F.COUNT:])
        assert not np.isfinite(d["z"][40, 0:3]).any()
    assert d["rec"][25, F.COUNT] == 6 and d["rec"][26, F.COUNT] == 4


# ---------------------------------------------------------------- 5: neutral loops
def _path1_fleet(nv, kind, faults, estimator, sigma=(0.05, 0.05, 0.005, 0.05)):
    from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop, ClosedLoopFrenet
    from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory
    from mkz_mpc_path_follower_amd.vehicle_sim import Estimator, SensorModel, VehicleSimulator, fault_params
    import scenario as S
    arr, lat0, lon0 = S.path_arrays("path1_decimated.npz")
    grt = GPSRefTrajectory(arrays=arr, traj_horizon=8, traj_dt=0.2, lat0=lat0, lon0=lon0)
    X0, Y0, P0, _ = LR.starts(nv)
    sim = VehicleSimulator(nv, X0=X0, Y0=Y0, Psi0=P0)
    sim.state[:, 3] = LR.VT
    kw = dict(sensor=SensorModel(nv, sigma=sigma, seed=3, faults=fault_params(nv) if faults else None))
    if estimator:
        kw.update(estimator=Estimator.from_sensor(kw["sensor"]))
    if kind == "frenet":
        return ClosedLoopFrenet(grt, sim, 8, LR.VT, **kw)
    return ClosedLoop(grt, sim, N=8, target_vel=LR.VT, **kw)


@pytest.mark.parametrize("estimator", [False, True])
@pytest.mark.parametrize("kind", ["cartesian", "frenet"])
def test_neutral_faulty_sensor_is_the_plain_sensor_in_the_loops(kind, estimator):
    """6 vehicles, 20 periods, noisy sensor: a neutral faulty sensor leaves the plain sensor's history bit for bit, with and without an estimator"""
    import torch
    plain_run = _path1_fleet(6, kind, False, estimator).run(20, history=True)
    loop = _path1_fleet(6, kind, True, estimator)
    full = loop.run(20, history=True)
    torch.cuda.synchronize()
    keys = ("state", "cmd", "status", "latch", "est") + (("est_filt",) if estimator else ())
    for k in keys:
        assert torch.equal(plain_run[k], full[k]), k
    assert torch.equal(plain_run["score"], full["score"]) and torch.equal(full["z"], full["est"]) and "z" not in plain_run and "fault_flags" not in plain_run
    assert (full["fault_flags"][0] == F.F_FRESH).all().item() and (full["fault_flags"][1:] == 0).all().item()
    assert tuple(full["z"].shape) == (20, 6, 4) and full["fault_flags"].dtype == torch.int32
    s = loop.sensor.fault_summary()
    assert (s["count"] == 20).all() and (s["n_silent_gps"] == 0).all() and s["count"].dtype == np.int64
    loop.sensor.reset_faults()
    assert not loop.sensor.fault_record.any().item()
    assert not torch.equal(full["est"], full["state"][:20, :, 0:4])         # the noise is there


# ---------------------------------------------------------------- 6, 7: the device loops against the CPU loops
LOOP_STEPS = 80
LOOP_ROWS = (F.window_row(30), F.window_row(10), F.NEUTRAL, F.window_row(15, start=40))


def _path3_loop(rows, estimator, blind_stop=False):
    from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop
    from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory
    from mkz_mpc_path_follower_amd.vehicle_sim import Estimator, SensorModel, VehicleSimulator
    import scenario as S
    nv = len(rows)
    arr, lat0, lon0 = S.path_arrays("path3_decimated.npz")
    grt = GPSRefTrajectory(arrays=arr, traj_horizon=8, traj_dt=0.2, lat0=lat0, lon0=lon0)
    tr, X0, Y0, P0 = F.path3()
    sim = VehicleSimulator(nv, X0=np.full(nv, X0), Y0=np.full(nv, Y0), Psi0=np.full(nv, P0))
    sim.state[:, 3] = F.VT
    kw = dict(sensor=SensorModel(nv, faults=np.array(rows)), blind_stop=blind_stop)
    if estimator:
        kw.update(estimator=Estimator(nv, q=F.EST_Q, r=F.EST_R))
    return tr, (X0, Y0, P0), ClosedLoop(grt, sim, N=8, target_vel=F.VT, **kw)


def _host(out, keys):
    import torch
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in keys}


@pytest.mark.parametrize("estimator", [False, True], ids=["held", "estimator"])
def test_loop_matches_the_cpu_loops(oracle, estimator):
    """4 vehicles from the ref tests' start on path3 at 6 m/s, 80 periods, no noise: GPS windows 20 ... 49, 20 ... 29, none, 40 ... 54, the
    controller reading the held state resp. an estimator fed z, against sensor_fault_ref.cpu_loop vehicle by vehicle.  NaN pattern, flags and
    latches equal.  Measured on the MI355X (MEASURED_LOOP): positions within 2.058e-11 m, the other states and the commands within 1.072e-10,
    the held state / estimate / finite z within 2.425e-11; bounds TOL_LOOP = 10 x, all below the 1e-6 cap.  Largest cross-track errors there:
    held fix 9.93 / 0.61 / 0.62 / 8.33 m, estimator 0.83 / 0.62 / 0.62 / 0.92 m (80 periods: the held-fix vehicle is still leaving the path)."""
    tr, (X0, Y0, P0), loop = _path3_loop(LOOP_ROWS, estimator)
    keys = ("state", "cmd", "status", "latch", "est", "z", "fault_flags") + (("est_filt",) if estimator else ())
    g = _host(loop.run(LOOP_STEPS, history=True), keys)
    assert (g["status"] == 0).all() and not g["latch"].any()
    worst = np.zeros(3)
    for b, row in enumerate(LOOP_ROWS):
        r = F.cpu_loop(oracle, tr, X0, Y0, P0, LOOP_STEPS, row, estimator=estimator, gid=b)
        assert (r["status"] == 0).all() and np.array_equal(g["fault_flags"][:, b], r["flags"]) and np.array_equal(np.isnan(g["z"][:, b]), np.isnan(r["z"]))
        dp = np.hypot(g["state"][:, b, 0] - r["state"][:, 0], g["state"][:, b, 1] - r["state"][:, 1]).max()
        do = max(np.abs(g["state"][:, b, 2:] - r["state"][:, 2:]).max(), np.abs(g["cmd"][:, b] - r["cmd"]).max())
        dz = max(np.abs(g["est"][:, b] - r["est"]).max(), np.nanmax(np.abs(g["z"][:, b] - r["z"])))
        if estimator:
            dz = max(dz, np.abs(g["est_filt"][:, b] - r["seen"]).max())
        print("vehicle %d against the CPU loop: max |dpos| = %.3e m, other states and commands %.3e, held, estimate and z %.3e" % (b, dp, do, dz))
        worst = np.maximum(worst, (dp, do, dz))
    print("worst: %s (bounds %s)" % (worst, TOL_LOOP))
    assert (worst <= TOL_LOOP).all() and TOL_LOOP.max() <= 1e-6
    e = [F.max_ect(tr, g["state"][:, b]) for b in range(4)]
    print("largest cross-track error [m], %s:" % ("estimator" if estimator else "held fix"), e)
    assert e[0] > 5.0 if not estimator else e[0] < 1.5


def test_blind_stop_latches_in_the_cpu_loops_periods(oracle):
    """4 vehicles, estimator, 40 periods, blind_stop: (window 10 from 20, MAX_AGE 5), (the same, MAX_AGE +inf), (window 10 from 22, MAX_AGE 3), neutral.
    The latch periods are the CPU loops' -- 25, never, 25, never -- and a latched vehicle is commanded -1.0 / 0.0.  blind_stop without a faulty
    sensor is refused."""
    from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop
    from mkz_mpc_path_follower_amd.vehicle_sim import SensorModel
    rows = (F.window_row(10, w14=5.0), F.window_row(10), F.window_row(10, start=22, w14=3.0), F.NEUTRAL)
    tr, (X0, Y0, P0), loop = _path3_loop(rows, True, blind_stop=True)
    g = _host(loop.run(40, history=True), ("cmd", "latch", "fault_flags", "state"))
    first = []
    for b, row in enumerate(rows):
        r = F.cpu_loop(oracle, tr, X0, Y0, P0, 40, row, estimator=True, blind_stop=True, gid=b)
        assert np.array_equal(g["latch"][:, b], r["latch"]) and np.array_equal(g["fault_flags"][:, b], r["flags"]), b
        first.append(int(np.argmax(r["latch"])) if r["latch"].any() else -1)
        assert (g["cmd"][:, b][g["latch"][:, b]] == np.array([-1.0, 0.0])).all() and (g["cmd"][:, b][~g["latch"][:, b], 0] != -1.0).all()
    assert first == [25, -1, 25, -1]
    assert loop.command_stop.cpu().numpy().tolist() == [True, False, True, False]
    for sensor in (None, SensorModel(4)):
        with pytest.raises(ValueError):
            ClosedLoop(loop.grt, loop.sim, N=8, target_vel=F.VT, sensor=sensor, blind_stop=True)
