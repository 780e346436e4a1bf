"""CPU side of the Monte-Carlo closed loop (a plant per vehicle, sensor noise, command delay): the numpy restatements of tests/plant_ref.py against
the oracle and against Random123's published answers, the host-side validation of plant rows and sensor rows, and the argument checks of the new
entry points, which all come before any device call."""
import ctypes as C

import numpy as np
import pytest

import plant_ref as R


def test_plant_ref_with_default_rows_is_the_oracle_bit_for_bit():
    from oracle import vehicle_sim as V
    s0, cmd = R.draw_states(np.random.default_rng(5), 300)
    assert (s0[:, 3] == 0).sum() > 10                                      # standing starts included
    got, held = R.update_plant(s0, cmd, np.tile(R.DEFAULT_ROW, (300, 1)), n_updates=10)
    assert np.array_equal(got, V.update_vehicle_model(s0, cmd, n_updates=10)) and np.array_equal(held, cmd)
    # a delay of 0 (or below) with any held command is no delay; a full-period delay is the held command for the whole period
    junk = np.full((300, 2), 0.3)
    assert np.array_equal(R.update_plant(s0, cmd, np.tile(R.DEFAULT_ROW, (300, 1)), 10, cmd_delay=np.full(300, -2), cmd_held=junk)[0], got)
    assert np.array_equal(R.update_plant(s0, cmd, np.tile(R.DEFAULT_ROW, (300, 1)), 10, cmd_delay=np.full(300, 25), cmd_held=junk)[0],
                          V.update_vehicle_model(s0, junk, n_updates=10))


def test_plant_default_row_is_the_reference():
    from mkz_mpc_path_follower_amd import _lib, vehicle_sim
    L = _lib.load()
    row = np.zeros(8)
    assert L.kmpc_plant_default(row.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert np.array_equal(row, R.DEFAULT_ROW) and vehicle_sim.PLANT_FIELDS == R.FIELDS and vehicle_sim.SENSOR_FIELDS == R.SENSOR_FIELDS
    assert L.kmpc_plant_default(None) == -1 and b"kmpc_plant_default" in L.kmpc_last_error(None)


def test_spread_case_stays_finite_and_away_from_the_unstable_band():
    """The inputs of the GPU test of per-vehicle rows.  The band where the 1 ms explicit Euler step of the linear-tyre model is unstable is
    vx < dt (C_f + C_r) / (2 m) <= 1e-3 * 1.3 * (4.0703e4 + 6.4495e4) / (2 * 0.7 * 1840) = 0.054 m/s at these spreads; every vehicle stays above 2 m/s.
    Slip-angle tangents: the draws of the existing kernel test (vy ~ N(0, 0.2), wz ~ N(0, 0.1), tyre angles up to 0.5) leave the kernel's polynomial
    range 1/8 at low speed whatever the seed (7 of these 300 vehicles start outside; the largest tangent over the period is 0.304), so the full case
    runs both the polynomials and, for those vehicles, the library's atan2 -- as the existing test does; the gentle case stays within 1/8 throughout
    (largest 0.031) and is the pure-polynomial one."""
    for gentle, lo, hi in ((False, 0.125, 0.5), (True, 0.0, 0.125)):
        s0, cmd, rows = R.spread_case(gentle)
        assert (np.abs(rows / R.DEFAULT_ROW - 1.0) <= 0.3 + 1e-15).all() and s0[:, 3].min() >= 2.0 and s0[:, 3].max() <= 20.0
        slip = []
        out, _ = R.update_plant(s0, cmd, rows, n_updates=10, slip=slip)
        assert np.isfinite(out).all() and out[:, 3].min() > 1.9
        assert lo <= slip[0] <= hi, slip
        for w in range(8):   # every word moves the state by 1000 x the GPU test's tolerance or more: there a swapped or ignored word cannot hide
            assert np.abs(out[291 + w] - out[290]).max() > 1e-6, (R.FIELDS[w], gentle)
        assert np.array_equal(out[290], out[299])


KNOWN_ANSWERS = [   # Random123, tests/kat_vectors: philox4x32 10
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("ctr,key,want", KNOWN_ANSWERS)
def test_philox_restatement_reproduces_the_known_answers(ctr, key, want):
    assert " ".join("%08x" % w for w in R.philox4x32_10(ctr, key)) == want


def test_sensor_restatement():
    """uniforms never 0 or 1; normals look normal; sigma 0 adds nothing; the heading wraps and the speed is floored"""
    n = np.array([R.normals(0x1234567800000001, g, p) for g in range(2000) for p in (0, 1)])
    assert np.isfinite(n).all() and np.abs(n).max() < 6.8 and abs(n.mean()) < 0.05 and abs(n.std() - 1.0) < 0.05
    assert abs(np.corrcoef(n[:-1, 0], n[1:, 0])[0, 1]) < 0.06
    hi = (0.5) * 2.0 ** -32
    assert np.sqrt(-2.0 * np.log(hi)) < 6.8 and (0xFFFFFFFF + 0.5) * 2.0 ** -32 < 1.0
    st = np.array([[1.0, 2.0, 3.0, 4.0], [1.0, 2.0, -3.0, 0.5]])
    rows = np.zeros((2, 8)); rows[:, 4:8] = [[0.25, -0.5, 0.5, -1.0], [0.0, 0.0, -0.5, -1.0]]
    est = R.sense(st, rows, 7, 3)
    assert np.array_equal(est[:, 0:2], st[:, 0:2] + rows[:, 4:6]) and (est[:, 3] == [3.0, 0.0]).all()
    assert abs(est[0, 2] - (3.5 - 2 * np.pi)) < 1e-15 and abs(est[1, 2] - (-3.5 + 2 * np.pi)) < 1e-15


def test_plant_params_validation():
    from mkz_mpc_path_follower_amd.vehicle_sim import check_plant_rows, plant_params
    p = plant_params(5, device="cpu", m=[1840.0, 2000.0, 2100.0, 2200.0, 2392.0], C_alpha_f=3.0e4)
    assert tuple(p.shape) == (5, 8) and p[4, 2].item() == 2392.0 and (p[:, 4] == 3.0e4).all().item() and np.array_equal(p[0, [0, 1, 3]].numpy(), R.DEFAULT_ROW[[0, 1, 3]])
    for bad in (dict(m=float("nan")), dict(m=0.0), dict(Iz=-1.0), dict(Iz=float("inf")), dict(lf=0.0), dict(lr=[1.0, 1.0, -1.0, 1.0, 1.0]),
                dict(C_alpha_f=0.0), dict(C_alpha_r=float("-inf")), dict(k_acc=-0.1), dict(k_df=float("nan")), dict(mass=1.0), dict(m=[1.0, 2.0])):
        with pytest.raises(ValueError):
            plant_params(5, device="cpu", **bad)
    plant_params(2, device="cpu", k_acc=0.0, k_df=0.0)       # a frozen actuator is a valid plant
    with pytest.raises(ValueError):
        check_plant_rows(np.ones((3, 7)))


def test_sensor_model_validation():
    from mkz_mpc_path_follower_amd.vehicle_sim import SensorModel
    s = SensorModel(3, sigma=(0.2, 0.2, 0.01, 0.1), bias=[[0.1, 0, 0, 0]] * 3, seed=2 ** 63 + 5, id_base=2 ** 40, device="cpu")
    assert tuple(s.params.shape) == (3, 8) and s.params[1].tolist() == [0.2, 0.2, 0.01, 0.1, 0.1, 0.0, 0.0, 0.0]
    for bad in (dict(sigma=-0.1), dict(sigma=float("nan")), dict(bias=float("inf")), dict(sigma=(1.0, 2.0)), dict(seed=-1), dict(seed=2 ** 64), dict(id_base=-1)):
        with pytest.raises(ValueError):
            SensorModel(3, device="cpu", **bad)


def test_new_symbols_are_exported_and_listed():
    from mkz_mpc_path_follower_amd import _lib
    L = _lib.load()
    for n in ("kmpc_plant_default", "kmpc_sim_advance_plant", "kmpc_sense_batch"):
        assert n in _lib.EXPORTS and hasattr(L, n), n
    assert L.kmpc_abi_version() == 8


def test_bad_arguments_are_refused_before_any_device_call():
    """every case answers KMPC_ERR_ARG without a GPU; the buffers are never read"""
    from mkz_mpc_path_follower_amd import _lib
    L = _lib.load()
    buf = C.cast(C.create_string_buffer(256), C.c_void_p)
    good = dict(B=2, state=buf, cmd=buf, plant=buf, delay=None, held=None, n=10)
    for c in (dict(B=-1), dict(n=-1), dict(state=None), dict(cmd=None), dict(plant=None), dict(delay=buf)):
        a = dict(good, **c)
        assert L.kmpc_sim_advance_plant(0, a["B"], a["state"], a["cmd"], a["plant"], a["delay"], a["held"], a["n"], None) == -1, c
        assert b"kmpc_sim_advance_plant" in L.kmpc_last_error(None)
    assert L.kmpc_sim_advance_plant(0, 0, None, None, None, None, None, 10, None) == 0      # B = 0: no launch
    assert L.kmpc_sim_advance_plant(0, 2, buf, buf, buf, buf, buf, 0, None) == 0            # no updates: no launch
    good = dict(B=2, state=buf, sensor=buf, period=0, id_base=0, est=buf)
    for c in (dict(B=-1), dict(state=None), dict(sensor=None), dict(est=None), dict(period=-1), dict(id_base=-1)):
        a = dict(good, **c)
        assert L.kmpc_sense_batch(0, a["B"], a["state"], a["sensor"], 1, a["period"], a["id_base"], a["est"], None) == -1, c
        assert b"kmpc_sense_batch" in L.kmpc_last_error(None)
    assert L.kmpc_sense_batch(0, 0, None, None, 1, 0, 0, None, None) == 0
