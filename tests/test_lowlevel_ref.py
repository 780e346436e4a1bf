"""CPU side of the low-level controller and the pedal-driven plant (kmpc_llc_default, kmpc_llc_step_batch, kmpc_drive_default,
kmpc_sim_advance_drive): the reference's own PidControl / LowPass numbers (tests/golden/lowlevel_classes.npz, recorded by
tools/make_lowlevel_fixture.py) against the numpy restatement tests/lowlevel_ref.py bit for bit, the symbols and their argument checks (no GPU
needed: every check comes before the first device call), the host validation, the conditions of the seeded cases the GPU tests use, and the physics
of the CPU closed loop that the GPU loop is compared with."""
import ctypes as C

import numpy as np
import pytest

import lowlevel_ref as LL
import plant_ref as R
import road_ref as RR

ARG = -1   # KMPC_ERR_ARG


# ---------------------------------------------------------------- the reference's classes
def test_restated_classes_reproduce_the_reference_bit_for_bit():
    """LowPass(0.5, 0.02).filt over 400 values and PidControl(0.8, 0.4, 0; 0 ... 1).step(e, 0.02) over 400 errors with 9 integrator resets, as the
    reference's headers computed them: lowpass_filt / pid_step give the same bits"""
    fx = LL.fixture()
    assert len(fx["lp_in"]) >= 400 and len(fx["pid_err"]) >= 400 and len(fx["pid_reset"]) >= 5
    last, ready, got = np.zeros(1), np.zeros(1), []
    for val in fx["lp_in"]:
        last, ready = LL.lowpass_filt(last, ready, np.array([val])), np.ones(1)
        got.append(last[0])
    assert np.array(got).tobytes() == fx["lp_out"].tobytes()
    kp, ki = fx["pid_params"][:2]
    integ, got, resets = np.zeros(1), [], set(fx["pid_reset"].tolist())
    for k, e in enumerate(fx["pid_err"]):
        if k in resets:
            integ = np.zeros(1)
        y, integ, _ = LL.pid_step(integ, np.array([e]), kp, ki)
        got.append(y[0])
    assert np.array(got).tobytes() == fx["pid_out"].tobytes()
    out = fx["pid_out"]
    assert (out == 1.0).sum() >= 10 and (out == 0.0).sum() >= 10 and ((out > 0) & (out < 1)).sum() >= 100     # the recording clips at both ends


def test_tick_replays_the_reference_bit_for_bit():
    """the same numbers through the whole tick, fed as tests/test_lowlevel.py feeds the kernel (lowlevel_ref.replay_lowpass / replay_pid)"""
    fx = LL.fixture()
    assert LL.replay_lowpass(LL.tick, fx).tobytes() == fx["lp_out"].tobytes()
    th, rec = LL.replay_pid(LL.tick, fx)
    assert th.tobytes() == fx["pid_out"].tobytes()
    assert rec[LL.TICKS] == len(th) and rec[LL.N_TH_SAT] == (fx["pid_out"] == 1.0).sum() and rec[LL.N_BRAKE] == 0 and rec[LL.N_DEADBAND] == 0


# ---------------------------------------------------------------- the library on a machine without a GPU
def test_symbols_default_rows_and_abi_version():
    from mkz_mpc_path_follower_amd import _lib
    from mkz_mpc_path_follower_amd import vehicle_sim as VS
    L = _lib.load()
    for name in ("kmpc_llc_default", "kmpc_llc_step_batch", "kmpc_drive_default", "kmpc_sim_advance_drive"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.kmpc_abi_version() == 8
    row = np.full(8, 7.0)
    assert L.kmpc_llc_default(row.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert row.tolist() == [0.8, 0.4, 1.0, 1.0, 14.8, 1847.78, 0.1, 0.33] and np.array_equal(row, LL.LLC_ROW)
    assert L.kmpc_llc_default(None) == ARG and b"kmpc_llc_default" in L.kmpc_last_error(None)
    row = np.full(8, 7.0)
    assert L.kmpc_drive_default(row.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert row.tolist() == [6000.0, 120e3, 5.0, 5.0, 0.15, 4e-4, 14.8, 0.33] and np.array_equal(row, LL.DRIVE_ROW)
    assert L.kmpc_drive_default(None) == ARG and b"kmpc_drive_default" in L.kmpc_last_error(None)
    assert np.array_equal(VS.llc_default(), LL.LLC_ROW) and np.array_equal(VS.drive_default(), LL.DRIVE_ROW)
    assert VS.LLC_FIELDS == LL.LLC_FIELDS and VS.DRIVE_FIELDS == LL.DRIVE_FIELDS and len(VS.LLC_RECORD_FIELDS) == 16


def test_argument_checks_answer_before_any_device_call():
    from mkz_mpc_path_follower_amd import _lib
    L = _lib.load()
    p = C.c_void_p(64)   # never dereferenced: every call below is refused on the host
    q = dict(B=2, cmd=p, speed=p, stride=8, llc=p, rec=p, out=p)

    def step(**kw):
        a = dict(q, **kw)
        return L.kmpc_llc_step_batch(0, a["B"], a["cmd"], a["speed"], a["stride"], a["llc"], a["rec"], a["out"], None)
    for bad in (dict(B=-1), dict(stride=0), dict(stride=-8), dict(cmd=None), dict(speed=None), dict(llc=None), dict(rec=None), dict(B=0, stride=0)):
        assert step(**bad) == ARG, bad
        assert b"kmpc_llc_step_batch" in L.kmpc_last_error(None)
    assert step(B=0) == 0 and step(B=0, cmd=None, speed=None, llc=None, rec=None, out=None) == 0     # nothing to do: success without a launch

    q = dict(B=2, state=p, cmd=p, plant=p, road=p, drive=p, llc=p, rec=p, delay=p, queue=p, depth=4, period=0, n=10, stat=p)

    def drive(**kw):
        a = dict(q, **kw)
        return L.kmpc_sim_advance_drive(0, a["B"], a["state"], a["cmd"], a["plant"], a["road"], a["drive"], a["llc"], a["rec"], a["delay"], a["queue"],
                                        a["depth"], a["period"], a["n"], a["stat"], None)
    for bad in (dict(B=-1), dict(n=-1), dict(state=None), dict(cmd=None), dict(plant=None), dict(road=None), dict(drive=None), dict(llc=None),
                dict(rec=None), dict(depth=1), dict(depth=0), dict(period=-1), dict(queue=None), dict(drive=None, stat=None)):
        assert drive(**bad) == ARG, bad
        assert b"kmpc_sim_advance_drive" in L.kmpc_last_error(None)
    assert drive(B=0) == 0 and drive(n=0) == 0 and drive(B=0, drive=None, llc=None, rec=None, stat=None) == 0
    assert drive(B=0, queue=None) == ARG and drive(n=0, depth=1) == ARG and drive(n=0, drive=None) == ARG and drive(n=0, rec=None) == ARG


def test_host_validation_without_a_gpu():
    import torch
    from mkz_mpc_path_follower_amd import vehicle_sim as VS
    r = VS.llc_params(3, device="cpu")
    assert r.dtype == torch.float64 and np.array_equal(r.numpy(), LL.llc_rows(3))
    r = VS.llc_params(3, device="cpu", brake_deadband=[0.0, 0.1, 0.2], mass=2000.0, kp=0.0)
    assert np.array_equal(r.numpy(), LL.llc_rows(3, brake_deadband=[0.0, 0.1, 0.2], mass=2000.0, kp=0.0))
    d = VS.drive_params(3, device="cpu", f_peak=[1500.0, 2500.0, 6000.0], c_roll=0.0)
    assert np.array_equal(d.numpy(), LL.drive_rows(3, f_peak=[1500.0, 2500.0, 6000.0], c_roll=0.0))
    nan, inf = float("nan"), float("inf")
    for bad in (dict(kp=-0.1), dict(ki=nan), dict(accel_max=0.0), dict(decel_max=-1.0), dict(steer_ratio=0.0), dict(mass=0.0), dict(mass=inf),
                dict(brake_deadband=-0.1), dict(wheel_radius=0.0), dict(kp=[0.8, 0.8]), dict(gain=1.0), dict(f_peak=1.0)):
        with pytest.raises(ValueError):
            VS.llc_params(3, device="cpu", **bad)
    for bad in (dict(f_peak=0.0), dict(f_peak=nan), dict(p_max=-1.0), dict(k_th=-1.0), dict(k_br=inf), dict(c_roll=-0.1), dict(c_drag=nan),
                dict(steer_ratio=0.0), dict(wheel_radius=0.0), dict(wheel_radius=[0.3, 0.3]), dict(mass=1.0)):
        with pytest.raises(ValueError):
            VS.drive_params(3, device="cpu", **bad)
    for w, v in ((0, -1.0), (1, nan), (2, 0.0), (3, 0.0), (4, -14.8), (5, 0.0), (6, -0.1), (7, 0.0), (7, inf)):
        rows = LL.llc_rows(3)
        rows[1, w] = v
        with pytest.raises(ValueError):
            VS.check_llc_rows(rows)
        with pytest.raises(ValueError):
            VS.LowLevelController(3, **{LL.LLC_FIELDS[w]: rows[:, w]})       # refused before the GPU is touched
    for w, v in ((0, 0.0), (1, 0.0), (2, -1.0), (3, nan), (4, -0.1), (5, -1e-4), (6, 0.0), (7, 0.0), (0, inf)):
        rows = LL.drive_rows(3)
        rows[1, w] = v
        with pytest.raises(ValueError):
            VS.check_drive_rows(rows)
        with pytest.raises(ValueError):
            VS.VehicleSimulator(3, drive=rows)                               # refused before the GPU is touched
    for shape in ((8,), (3, 4), (2, 3, 8)):
        with pytest.raises(ValueError):
            VS.check_drive_rows(np.ones(shape))
        with pytest.raises(ValueError):
            VS.check_llc_rows(np.ones(shape))
    for rows in (LL.drive_rows(2), LL.drive_rows(3)[:, :6]):
        with pytest.raises(ValueError):
            VS.VehicleSimulator(3, drive=rows)
    with pytest.raises(ValueError):
        VS.VehicleSimulator(3, llc=object())                                 # llc= without drive=
    with pytest.raises(ValueError):
        VS.VehicleSimulator(3, drive=LL.drive_rows(3), llc=object())
    with pytest.raises(ValueError):
        VS.LowLevelController(3, v0=[6.0, 6.0])
    assert VS.check_llc_rows(LL.random_llc_rows()) is not None and VS.check_drive_rows(LL.random_drive_rows()) is not None


# ---------------------------------------------------------------- what the tick does
def test_tick_branches_by_hand():
    """one controller from a fresh record at rest: the first report passes unfiltered, throttle = KP e with an empty integrator, the deadband gives
    neither pedal and resets the integrator, below it the brake torque is -a m r, the clamps and the steering-wheel limit hold"""
    par = LL.llc_rows(1)
    rec, ped = LL.tick(np.zeros((1, 16)), par, [0.0], [[0.5, 0.1]])
    assert ped[0].tolist() == [0.8 * 0.5, 0.0, 0.1 * 14.8, 0.5] and rec[0, LL.INT] == 0.5 * 0.02 and rec[0, LL.READY] == 1.0
    rec, ped = LL.tick(rec, par, [0.01], [[0.5, 0.1]])                        # raw = 0.5 m/s^2, filtered: a * 0.5 + b * 0
    lpf = LL.LP_A * (50.0 * 0.01)
    assert rec[0, LL.LPF] == lpf and ped[0, 0] == 0.8 * (0.5 - lpf) + 0.4 * (0.5 * 0.02)
    rec, ped = LL.tick(rec, par, [0.01], [[-0.05, 0.0]])
    assert ped[0].tolist() == [0.0, 0.0, 0.0, -0.05] and rec[0, LL.INT] == 0.0 and rec[0, LL.N_DEADBAND] == 1 and rec[0, LL.N_BRAKE] == 0
    rec, ped = LL.tick(rec, par, [0.01], [[-0.5, 0.0]])
    assert ped[0, 1] == 0.5 * 1847.78 * 0.33 and ped[0, 0] == 0.0 and rec[0, LL.N_BRAKE] == 1
    rec, ped = LL.tick(rec, par, [0.01], [[-7.0, -0.9]])
    assert ped[0, 3] == -1.0 and ped[0, 1] == 1.0 * 1847.78 * 0.33 and ped[0, 2] == -8.2
    rec, ped = LL.tick(rec, par, [0.01], [[7.0, 0.9]])
    assert ped[0, 3] == 1.0 and ped[0, 2] == 8.2 and rec[0, LL.TICKS] == 6
    rec, ped = LL.tick(rec, LL.llc_rows(1, kp=5.0), [0.01], [[1.0, 0.0]])
    assert ped[0, 0] == 1.0 and rec[0, LL.N_TH_SAT] == 1
    assert rec[0, LL.MAX_ERR] > 0 and rec[0, LL.SUM_ERR2] >= rec[0, LL.MAX_ERR] ** 2


def test_what_the_pedals_deliver_in_steady_state():
    """default rows, straight ahead from 6 m/s, a constant command for 6 s: the acceleration that the plant's word 6 settles at.  A command inside the
    deadband coasts on the resistances (0.15 + 4e-4 v^2), a brake command is the brake law's -a m_est / m plus the resistances it does not know of,
    a throttle command is delivered (the PI loop closes on the measured acceleration).  The issue's prototype: -0.05 -> -0.16, -1.0 -> -1.16."""
    B = 3
    cmdv = np.array([-0.05, -1.0, 0.5])
    s = np.zeros((B, 8))
    s[:, 3] = 6.0
    rec = np.zeros((B, 16))
    rec[:, LL.V_LAST] = 6.0
    plant, road, drive, llc = np.tile(R.DEFAULT_ROW, (B, 1)), RR.rows(B), LL.drive_rows(B), LL.llc_rows(B)
    cmd = np.stack([cmdv, np.zeros(B)], 1)
    accs = []
    for p in range(60):
        s, rec, _ = LL.update_drive(s, cmd, plant, road, drive, llc, rec, p, 10)
        accs.append(s[:, 6].copy())
        if p == 19:
            early = s.copy()
    print("steady state: commanded", cmdv, "-> acc after 2 s", accs[19], "speeds", early[:, 3], "; after 6 s", s[:, 6], "speeds", s[:, 3])
    v = early[:, 3]
    assert abs(accs[19][0] + (0.15 + 4e-4 * v[0] ** 2)) < 1e-6 and rec[0, LL.N_DEADBAND] == rec[0, LL.TICKS] and rec[0, LL.N_BRAKE] == 0
    assert abs(accs[19][1] + (1847.78 / 1840.0 + 0.15 + 4e-4 * v[1] ** 2)) < 1e-3 and rec[1, LL.N_BRAKE] == rec[1, LL.TICKS]
    assert abs(accs[19][0] + 0.16) < 0.01 and abs(accs[19][1] + 1.16) < 0.01
    assert abs(accs[59][2] - 0.5) < 0.02 and rec[2, LL.N_TH_SAT] == 0
    assert s[1, 3] == 0.0 and s[1, 6] < 0.0                                   # the braked car stopped and stays


# ---------------------------------------------------------------- the seeded cases of the GPU tests
def test_stage_case_visits_every_branch_and_none_narrowly():
    """tests/test_lowlevel.py's stage case compares bit for bit, so nearness cannot hurt it; the case must still visit every branch"""
    rows, v, cmds, rec = LL.stage_case()
    B = rows.shape[0]
    assert B == 300 and v.shape == (50, B) and (v >= 0).all() and not rec[:10].any()
    near = np.zeros(B, dtype=bool)
    clamp_hi = clamp_lo = wheel = 0
    for k in range(len(v)):
        rec, ped = LL.tick(rec, rows, v[k], cmds[k], near=near)
        clamp_hi += (ped[:, 3] == rows[:, 2]).sum()
        clamp_lo += (ped[:, 3] == -rows[:, 3]).sum()
        wheel += (np.abs(ped[:, 2]) == 8.2).sum()
    print("stage case: near a branch %d; N_TH_SAT %d, N_DEADBAND %d, N_BRAKE %d, clamped high %d low %d, wheel limit %d, throttle inside (0, 1) %d"
          % (near.sum(), rec[:, LL.N_TH_SAT].sum(), rec[:, LL.N_DEADBAND].sum(), rec[:, LL.N_BRAKE].sum(), clamp_hi, clamp_lo, wheel,
             ((rec[:, LL.TH_CMD] > 0) & (rec[:, LL.TH_CMD] < 1)).sum()))
    assert not near.any() and np.isfinite(rec).all()
    assert min(rec[:, LL.N_TH_SAT].sum(), rec[:, LL.N_DEADBAND].sum(), rec[:, LL.N_BRAKE].sum(), clamp_hi, clamp_lo, wheel) >= 50
    assert (rec[:, LL.TICKS] == 50).all() and (rec[:, LL.INT] != 0).sum() >= 50


@pytest.mark.parametrize("n", [10, 7])
def test_drive_case_has_no_vehicle_near_a_branch(n):
    """the one-period case of the GPU test, periods 0 ... 3: no restated PI output within 1e-9 of 0 or 1 and no command within 1e-9 of 0, the
    deadband or a clamp -- the GPU test's counters are then exact for every vehicle -- and the rows are valid and the pedals do act"""
    s, cmd, plant, road, drive, llc, rec = LL.drive_case()
    B = len(s)
    near, stat = np.zeros(B, dtype=bool), np.zeros((B, 4))
    cmds = np.tile(cmd, (4, 1, 1))
    for p in range(4):
        s, rec, stat = LL.advance_drive(s, cmds, p, plant, road, drive, llc, rec, np.zeros(B, dtype=np.int64), 2, n, stat=stat, near=near)
    ticks = (4 * n + 1) // 2
    print("drive case n = %d: near a branch %d; N_TH_SAT > 0 in %d vehicles, N_DEADBAND in %d, N_BRAKE in %d" %
          (n, near.sum(), (rec[:, LL.N_TH_SAT] > 0).sum(), (rec[:, LL.N_DEADBAND] > 0).sum(), (rec[:, LL.N_BRAKE] > 0).sum()))
    assert not near.any() and np.isfinite(s).all() and np.isfinite(rec).all() and (rec[:, LL.TICKS] == ticks).all()
    assert min((rec[:, LL.N_TH_SAT] > 0).sum(), (rec[:, LL.N_DEADBAND] > 0).sum(), (rec[:, LL.N_BRAKE] > 0).sum()) >= 10


def test_tick_phase_does_not_depend_on_how_the_updates_are_cut():
    """40 updates as 4 x 10 and as 8 x 5 under one command: the same state and record bit for bit (the tick runs on even ABSOLUTE updates)"""
    s, cmd, plant, road, drive, llc, rec = LL.drive_case()
    a, ra, b, rb = s, rec, s, rec
    for p in range(4):
        a, ra, _ = LL.update_drive(a, cmd, plant, road, drive, llc, ra, p, 10)
    for p in range(8):
        b, rb, _ = LL.update_drive(b, cmd, plant, road, drive, llc, rb, p, 5)
    assert a.tobytes() == b.tobytes() and ra.tobytes() == rb.tobytes() and (ra[:, LL.TICKS] == 20).all()


# ---------------------------------------------------------------- the closed loop
def test_cpu_loop_shows_deadband_saturation_and_mass_error(oracle):
    """six vehicles on path3 from 58 % of its length, already at 6 m/s, 120 periods (lowlevel_ref.LOOP_OFFSETS): default rows; BRAKE_DEADBAND 0; F_PEAK
    500 N; plant mass x 1.3; the first two also 0.3 m beside the path.  Every state finite, every solve Optimal; the default vehicle spends ticks in
    the deadband and the zero-deadband one none; the weak engine saturates the throttle and ends slower than the default."""
    runs, _tr = LL.cpu_loops(oracle)
    for b, ((row, off), r) in enumerate(zip(LL.LOOP_OFFSETS, runs)):
        rec = r["rec"]
        print("cpu loop vehicle %d (%s, %.1f m beside): final speed %.4f m/s, mean %.4f; ticks %d, throttle saturated %d, deadband %d, brake %d, rms(ac - a) %.4f%s"
              % (b, LL.LOOP_ROWS[row] or "default", off, r["state"][-1, 3], r["state"][60:, 3].mean(), rec[LL.TICKS], rec[LL.N_TH_SAT], rec[LL.N_DEADBAND],
                 rec[LL.N_BRAKE], np.sqrt(rec[LL.SUM_ERR2] / rec[LL.TICKS]), "; near a branch" if r["near"] else ""))
        assert np.isfinite(r["state"]).all() and np.isfinite(rec).all() and (r["status"] == 0).all() and rec[LL.TICKS] == 600
    assert runs[0]["rec"][LL.N_DEADBAND] > 0 and runs[1]["rec"][LL.N_DEADBAND] > 0
    assert runs[2]["rec"][LL.N_DEADBAND] == 0 and runs[3]["rec"][LL.N_DEADBAND] == 0
    assert runs[4]["rec"][LL.N_TH_SAT] > 0 and runs[4]["state"][-1, 3] < runs[0]["state"][-1, 3]
