"""The refusal texts of the loop stages' host plumbing, as a table: (call, bad argument, the exact text of the ValueError).

Every text below is a literal, written down from the code as it stood before the stages' tensor contract and row tables were given one
implementation each.  INTEGRATION.md tells callers to read these texts, so they are a public contract: a helper that serves several stages must
leave each stage its own words and its own order of checks.  Each case only raises: every check here answers before the library is called, so the
CPU part needs no device and the `gpu` part launches nothing.

The CPU part builds the stages with device="cpu" (as tests/test_predict_dist_ref.py does) for B = 3 vehicles; the `gpu` part covers what needs a
device to construct, on a two-path fleet of the fixture paths.

The fleet stages (RangeSensor, Follower, Lanes, SpeedPlanner.plan's state and v_cap, check_search, the loops' planner= / follower= / lanes=
checks) were written down the same way, from the code as it stood before they were given one state-view rule, one v_cap / out pair and one base
class; where two things are wrong at once the case names the text that must win.
"""
import types

import numpy as np
import pytest

B = 3
PLANT = "lf, lr, m, Iz, C_alpha_f, C_alpha_r, k_acc, k_df"
ROAD = "mu_f, mu_r, a_long, a_lat, df_offset, acc_gain"
FAULT = ("p_lose_gps, p_lose_imu, p_lose_spd, p_regain_gps, p_regain_imu, p_regain_spd, win_from_gps, win_from_imu, win_from_spd, win_len_gps, "
         "win_len_imu, win_len_spd, p_outlier, outlier_sigma, max_age")
LLC = "kp, ki, accel_max, decel_max, steer_ratio, mass, brake_deadband, wheel_radius"
DRIVE = "f_peak, p_max, k_th, k_br, c_roll, c_drag, steer_ratio, wheel_radius"
PLAN = "a_lat, a_brake, v_floor, end_stop"


def refused(cases):
    """every (name, call, text): call() must raise a ValueError whose text is exactly `text`; all the misses are reported together"""
    bad = []
    for name, call, text in cases:
        try:
            call()
        except ValueError as e:
            if str(e) != text:
                bad.append("%s:\n  expected %r\n  got      %r" % (name, text, str(e)))
        except Exception as e:   # noqa: BLE001 -- the table states which exception it is
            bad.append("%s: %s instead of a ValueError: %s" % (name, type(e).__name__, e))
        else:
            bad.append("%s: accepted" % name)
    assert not bad, "\n".join(bad)


def swapped(obj, attr, value, call):
    """call() while obj.attr is `value` (a public tensor replaced by the caller); the attribute is put back afterwards"""
    def run():
        keep = getattr(obj, attr)
        setattr(obj, attr, value)
        try:
            call()
        finally:
            setattr(obj, attr, keep)
    return run


def f64(*shape):
    import torch
    return torch.zeros(shape, dtype=torch.float64)


def strided(w, rows=B):
    """[rows,w] float64, the right shape but not contiguous"""
    return f64(w, rows).t()


def test_wander_sensor_and_llc_contracts():
    import torch
    from mkz_mpc_path_follower_amd.vehicle_sim import LowLevelController, SensorModel, Wander, wander_rows
    w = Wander(B, wander_rows(B), device="cpu")
    row = "%s: a contiguous float64 tensor [3,%d] on cpu"
    sen = SensorModel(B, device="cpu")
    sense = "state [B,8], params [B,8] and est [B,4] must be contiguous float64 tensors on cpu"
    llc = LowLevelController(B, device="cpu")
    own = "params [B,8] and rec [B,16] must stay contiguous float64 tensors on cpu (write into them with copy_)"
    bufs = "cmd [B,2] and out [B,4] must be contiguous float64 tensors on cpu"
    speed = "speed: float64 [B] on cpu, rows a fixed distance >= 1 apart (a [B] buffer or sim.state[:, 3])"
    refused([
        ("wander params replaced", swapped(w, "params", w.params.float(), lambda: w.step(0)), row % ("params", 24)),
        ("wander rec transposed", swapped(w, "rec", strided(16), lambda: w.step(0)), row % ("rec", 16)),
        ("wander sensor_base numpy", lambda: w.step(0, np.zeros((B, 8)), f64(B, 8)), row % ("sensor_base", 8)),
        ("wander sensor_out dtype", lambda: w.step(0, f64(B, 8), f64(B, 8).float()), row % ("sensor_out", 8)),
        ("wander road_base shape", lambda: w.step(0, None, None, f64(B, 6), f64(B, 8)), row % ("road_base", 8)),
        ("wander road_out strided", lambda: w.step(0, None, None, f64(B, 8), strided(8)), row % ("road_out", 8)),
        ("sense state dtype", lambda: sen.sense(f64(B, 8).float(), 0), sense),
        ("sense state shape", lambda: sen.sense(f64(B, 6), 0), sense),
        ("sense state strided", lambda: sen.sense(strided(8), 0), sense),
        ("sense state numpy", lambda: sen.sense(np.zeros((B, 8)), 0), sense),
        ("sense params replaced", swapped(sen, "params", sen.params.float(), lambda: sen.sense(f64(B, 8), 0)), sense),
        ("sense out shape", lambda: sen.sense(f64(B, 8), 0, out=f64(B, 3)), sense),
        ("llc params replaced", swapped(llc, "params", llc.params.float(), lambda: llc.step(f64(B, 2), f64(B))), own),
        ("llc rec numpy", swapped(llc, "rec", np.zeros((B, 16)), lambda: llc.step(f64(B, 2), f64(B))), own),
        ("llc cmd dtype", lambda: llc.step(f64(B, 2).float(), f64(B)), bufs),
        ("llc cmd strided", lambda: llc.step(strided(2), f64(B)), bufs),
        ("llc cmd numpy", lambda: llc.step(np.zeros((B, 2)), f64(B)), bufs),
        ("llc out shape", lambda: llc.step(f64(B, 2), f64(B), out=f64(B, 3)), bufs),
        ("llc speed stride 0", lambda: llc.step(f64(B, 2), f64(1).expand(B)), speed),
        ("llc speed shape", lambda: llc.step(f64(B, 2), f64(B, 1)), speed),
        ("llc speed dtype", lambda: llc.step(f64(B, 2), f64(B).float()), speed),
        ("llc speed numpy", lambda: llc.step(f64(B, 2), np.zeros(B)), speed),
    ])
    assert torch.equal(w.params, torch.zeros((B, 24), dtype=torch.float64)) and llc.rec.dtype == torch.float64   # the swaps were undone


def test_estimator_and_observer_contracts():
    import torch
    from mkz_mpc_path_follower_amd.vehicle_sim import DisturbanceObserver, Estimator
    est, ob = Estimator(B, device="cpu"), DisturbanceObserver(B, device="cpu")
    ebuf = "z [B,4], params [B,8], record [B,16], est [B,4] and innov [B,4] must be contiguous float64 tensors on cpu"
    obuf = "z [B,4], est [B,4], innov [B,4] and dist [B,3] must be contiguous float64 tensors on cpu"
    own = "params [B,16] and record [B,40] must stay contiguous float64 tensors on cpu"
    flags = "flags must stay a contiguous int32 tensor [B] on cpu"
    u_text = "u: float64 [B,2] on cpu with unit column stride and rows >= 2 apart (a [B,2] buffer or sim.state[:, 6:8])"
    cmd = "cmd must be a contiguous float64 tensor [B,2] on cpu"
    latch = "stop_latch must be a contiguous bool or uint8 tensor [B] on cpu"
    bad_u = (("column stride 2", f64(B, 4)[:, ::2]), ("transposed", f64(2, B).t()), ("rows 1 apart", torch.as_strided(f64(B + 1), (B, 2), (1, 1))),
             ("dtype", f64(B, 2).float()), ("shape", f64(B, 3)), ("numpy", np.zeros((B, 2))))
    cases = []
    for name, o, buf in (("estimator", est, ebuf), ("observer", ob, obuf)):
        up = o.update
        cases += [
            (name + " z dtype", lambda up=up: up(f64(B, 4).float(), f64(B, 2)), buf),
            (name + " z shape", lambda up=up: up(f64(B, 3), f64(B, 2)), buf),
            (name + " z strided", lambda up=up: up(strided(4), f64(B, 2)), buf),
            (name + " z numpy", lambda up=up: up(np.zeros((B, 4)), f64(B, 2)), buf),
            (name + " out shape", lambda up=up: up(f64(B, 4), f64(B, 2), out=f64(B, 8)), buf),
            (name + " innov replaced", swapped(o, "innov", o.innov.float(), lambda up=up: up(f64(B, 4), f64(B, 2))), buf),
            (name + " flags replaced", swapped(o, "flags", o.flags.long(), lambda up=up: up(f64(B, 4), f64(B, 2))), flags),
            (name + " flags shape", swapped(o, "flags", torch.zeros((B, 1), dtype=torch.int32), lambda up=up: up(f64(B, 4), f64(B, 2))), flags),
        ]
        cases += [("%s u %s" % (name, what), lambda up=up, u=u: up(f64(B, 4), u), u_text) for what, u in bad_u]
    cases += [
        ("estimator params replaced", swapped(est, "params", est.params.float(), lambda: est.update(f64(B, 4), f64(B, 2))), ebuf),
        ("estimator record transposed", swapped(est, "record", strided(16), lambda: est.update(f64(B, 4), f64(B, 2))), ebuf),
        ("observer params replaced", swapped(ob, "params", ob.params.float(), lambda: ob.update(f64(B, 4), f64(B, 2))), own),
        ("observer record transposed", swapped(ob, "record", strided(40), lambda: ob.update(f64(B, 4), f64(B, 2))), own),
        ("observer dist replaced", swapped(ob, "dist", ob.dist.float(), lambda: ob.update(f64(B, 4), f64(B, 2))), obuf),
        ("observer own before its buffers", swapped(ob, "params", ob.params.float(), lambda: ob.update(f64(B, 3), f64(B, 2))), own),
        ("offset record replaced", swapped(ob, "record", ob.record.float(), lambda: ob.offset(f64(B, 2))), own),
        ("offset cmd dtype", lambda: ob.offset(f64(B, 2).float()), cmd),
        ("offset cmd shape", lambda: ob.offset(f64(B, 3)), cmd),
        ("offset cmd strided", lambda: ob.offset(strided(2)), cmd),
        ("offset cmd numpy", lambda: ob.offset(np.zeros((B, 2))), cmd),
        ("offset latch dtype", lambda: ob.offset(f64(B, 2), torch.zeros(B, dtype=torch.int32)), latch),
        ("offset latch shape", lambda: ob.offset(f64(B, 2), torch.zeros(B + 1, dtype=torch.bool)), latch),
        ("offset latch strided", lambda: ob.offset(f64(B, 2), torch.zeros(2 * B, dtype=torch.uint8)[::2]), latch),
        ("offset latch numpy", lambda: ob.offset(f64(B, 2), np.zeros(B, dtype=np.uint8)), latch),
    ]
    refused(cases)


def test_latency_compensator_contracts():
    import torch
    from mkz_mpc_path_follower_amd.vehicle_sim import DisturbanceObserver, LatencyCompensator
    comp = LatencyCompensator(B, cmd_delay=25, meas_delay=1, device="cpu", disturbances=True)
    ob = DisturbanceObserver(B, device="cpu")
    own = "cmd_delay, meas_delay [B] int32 and cmd_hist [depth,B,2] float64 must stay contiguous tensors on cpu"
    buf = "%s must be a contiguous float64 tensor [B,%d] on cpu"
    refused([
        ("cmd_delay replaced", swapped(comp, "cmd_delay", comp.cmd_delay.long(), lambda: comp.predict(f64(B, 4), 0)), own),
        ("meas_delay numpy", swapped(comp, "meas_delay", np.zeros(B, dtype=np.int32), lambda: comp.filter_input(0)), own),
        ("cmd_hist transposed", swapped(comp, "cmd_hist", comp.cmd_hist.transpose(0, 1), lambda: comp.push(f64(B, 2), 0)), own),
        ("period", lambda: comp.predict(f64(B, 4), -1), "period >= 0"),
        ("predict z dtype", lambda: comp.predict(f64(B, 4).float(), 0), buf % ("z", 4)),
        ("predict z strided", lambda: comp.predict(strided(4), 0), buf % ("z", 4)),
        ("predict z numpy", lambda: comp.predict(np.zeros((B, 4)), 0), buf % ("z", 4)),
        ("predict out shape", lambda: comp.predict(f64(B, 4), 0, out=f64(B, 3)), buf % ("out", 4)),
        ("filter_input out shape", lambda: comp.filter_input(0, out=f64(B, 4)), buf % ("out", 2)),
        ("push cmd shape", lambda: comp.push(f64(B, 3), 0), buf % ("cmd", 2)),
        ("predict_disturbed est", lambda: comp.predict_disturbed(ob, f64(B, 3), 0), buf % ("est", 4)),
        ("predict_disturbed out", lambda: comp.predict_disturbed(ob, f64(B, 4), 0, out=f64(B, 4).float()), buf % ("out", 4)),
        ("predict_disturbed observer's own", swapped(ob, "record", ob.record.float(), lambda: comp.predict_disturbed(ob, f64(B, 4), 0)),
         "params [B,16] and record [B,40] must stay contiguous float64 tensors on cpu"),
    ])
    assert comp.cmd_delay.dtype == torch.int32


def test_stage_constructor_blocks():
    """a scalar, w values or [B,w] into a block of the row; gate, dt, L_a, L_b"""
    from mkz_mpc_path_follower_amd.vehicle_sim import DisturbanceObserver, Estimator, SensorModel
    four = "%s: %s is a scalar, four values (x, y, psi, v) or [3,4], got %s"
    scal = "%s: gate >= 0, dt > 0, L_a > 0, L_b > 0, all finite (got %s)"
    refused([
        ("sensor sigma", lambda: SensorModel(B, sigma=(1.0, 2.0, 3.0), device="cpu"), four % ("SensorModel", "sigma", "(3,)")),
        ("sensor bias", lambda: SensorModel(B, bias=np.zeros((2, 4)), device="cpu"), four % ("SensorModel", "bias", "(2, 4)")),
        ("sensor sign", lambda: SensorModel(B, sigma=-1.0, device="cpu"), "SensorModel: sigma and bias must be finite, sigma >= 0"),
        ("estimator q", lambda: Estimator(B, q=(1.0, 2.0), device="cpu"), four % ("Estimator", "q", "(2,)")),
        ("estimator r", lambda: Estimator(B, r=np.ones((B, 3)), device="cpu"), four % ("Estimator", "r", "(3, 3)")),
        ("estimator r sign", lambda: Estimator(B, r=0.0, device="cpu"), "Estimator: q and r must be finite, q >= 0, r > 0"),
        ("estimator dt", lambda: Estimator(B, dt=0, device="cpu"), scal % ("Estimator", "0.0, 0, 1.108, 1.742")),
        ("estimator gate", lambda: Estimator(B, gate=-1.0, device="cpu"), scal % ("Estimator", "-1.0, 0.1, 1.108, 1.742")),
        ("observer q", lambda: DisturbanceObserver(B, q=(1.0, 2.0), device="cpu"), "DisturbanceObserver: q is a scalar, 4 values or [3,4], got (2,)"),
        ("observer q_dist", lambda: DisturbanceObserver(B, q_dist=(1.0, 2.0, 3.0, 4.0), device="cpu"),
         "DisturbanceObserver: q_dist is a scalar, 3 values or [3,3], got (4,)"),
        ("observer p0", lambda: DisturbanceObserver(B, p0=np.ones((B, 4)), device="cpu"), "DisturbanceObserver: p0 is a scalar, 3 values or [3,3], got (3, 4)"),
        ("observer sign", lambda: DisturbanceObserver(B, r=0.0, device="cpu"),
         "DisturbanceObserver: q, q_dist, r and p0 must be finite, q >= 0, q_dist >= 0, r > 0, p0 >= 0"),
        ("observer L_a", lambda: DisturbanceObserver(B, L_a=float("inf"), device="cpu"), scal % ("DisturbanceObserver", "0.0, 0.1, inf, 1.742")),
        ("observer caps", lambda: DisturbanceObserver(B, df_cap=-0.1, device="cpu"),
         "DisturbanceObserver: v_min, psi_cap, acc_cap, df_cap >= 0, all finite (got 1.0, 0.2, 0.5, -0.1)"),
    ])


def test_row_tables():
    """one unknown key, one wrong-length override and one group-plus-member conflict for every *_params; what the check_*_rows share"""
    from mkz_mpc_path_follower_amd import ref_traj as RT, vehicle_sim as VS
    unknown = "%s: unknown parameter 'bogus' (one of %s)"
    length = "%s: %s is a scalar or one value per vehicle [3], got (2,)"
    groups = "p_lose, p_regain, win_from, win_len"
    both = "road_params: mu= sets both axles; give mu_f= and mu_r= instead of combining them with it"
    three = "fault_params: %s= sets all three sources; give the per-source words instead of combining them with it"
    cases = []
    for name, fn, fields, key in (("plant_params", VS.plant_params, PLANT, "m"), ("llc_params", VS.llc_params, LLC, "kp"),
                                  ("drive_params", VS.drive_params, DRIVE, "c_drag"), ("speed_plan_params", RT.speed_plan_params, PLAN, "a_brake")):
        cases += [(name + " unknown", lambda fn=fn: fn(B, device="cpu", bogus=1.0), unknown % (name, fields)),
                  (name + " length", lambda fn=fn, key=key: fn(B, device="cpu", **{key: [1.0, 2.0]}), length % (name, key)),
                  (name + " matrix", lambda fn=fn, key=key: fn(B, device="cpu", **{key: np.ones((B, 1))}),
                   "%s: %s is a scalar or one value per vehicle [3], got (3, 1)" % (name, key))]
    cases += [
        ("LowLevelController unknown", lambda: VS.LowLevelController(B, device="cpu", bogus=1.0), unknown % ("LowLevelController", LLC)),
        ("LowLevelController length", lambda: VS.LowLevelController(B, device="cpu", mass=[1.0, 2.0]), length % ("LowLevelController", "mass")),
        ("LowLevelController v0", lambda: VS.LowLevelController(B, device="cpu", v0=[1.0, 2.0]),
         "LowLevelController: v0 is a finite scalar or one speed per vehicle [3]"),
        ("road_params unknown", lambda: VS.road_params(B, device="cpu", bogus=1.0), "road_params: unknown parameter 'bogus' (mu or one of %s)" % ROAD),
        ("road_params length", lambda: VS.road_params(B, device="cpu", mu=[0.5, 0.4]), length % ("road_params", "mu")),
        ("road_params member length", lambda: VS.road_params(B, device="cpu", a_lat=[0.5, 0.4]), length % ("road_params", "a_lat")),
        ("road_params mu with mu_f", lambda: VS.road_params(B, device="cpu", mu=0.5, mu_f=0.4), both),
        ("road_params mu_r then mu", lambda: VS.road_params(B, device="cpu", mu_r=0.4, mu=0.5), both),
        ("fault_params unknown", lambda: VS.fault_params(B, device="cpu", bogus=1.0),
         "fault_params: unknown parameter 'bogus' (%s or one of %s)" % (groups, FAULT)),
        ("fault_params length", lambda: VS.fault_params(B, device="cpu", win_len=[1.0, 2.0]), length % ("fault_params", "win_len")),
        ("fault_params member length", lambda: VS.fault_params(B, device="cpu", p_outlier=[0.1, 0.2]), length % ("fault_params", "p_outlier")),
        ("fault_params p_lose with p_lose_gps", lambda: VS.fault_params(B, device="cpu", p_lose=0.1, p_lose_gps=0.2), three % "p_lose"),
        ("fault_params p_regain with p_regain_spd", lambda: VS.fault_params(B, device="cpu", p_regain_spd=0.2, p_regain=0.1), three % "p_regain"),
        ("fault_params win_from with win_from_imu", lambda: VS.fault_params(B, device="cpu", win_from=1, win_from_imu=2), three % "win_from"),
        ("fault_params win_len with win_len_gps", lambda: VS.fault_params(B, device="cpu", win_len=1, win_len_gps=2), three % "win_len"),
        # the validation that follows the table: one text of each check_*_rows, with the listing of the offending vehicles
        ("plant_params value", lambda: VS.plant_params(B, device="cpu", m=[1.0, -1.0, 0.0]),
         "plant rows: lf, lr, m, Iz, C_alpha_f, C_alpha_r must be > 0 (vehicle(s) [1, 2])"),
        ("road_params value", lambda: VS.road_params(B, device="cpu", mu=[0.5, 0.0, 1.0]), "road rows: mu_f, mu_r must be > 0 (+inf: no limit) (vehicle(s) [1])"),
        ("fault_params value", lambda: VS.fault_params(B, device="cpu", p_lose=[0.5, 0.0, 1.5]),
         "fault rows: p_lose_*, p_regain_* and p_outlier are probabilities in [0, 1] (vehicle(s) [2])"),
        ("llc_params value", lambda: VS.llc_params(B, device="cpu", mass=[0.0, 1.0, 1.0]),
         "llc rows: accel_max, decel_max, steer_ratio, mass, wheel_radius must be > 0 (vehicle(s) [0])"),
        ("drive_params value", lambda: VS.drive_params(B, device="cpu", c_drag=[0.0, 1.0, -1.0]),
         "drive rows: k_th, k_br, c_roll, c_drag must be >= 0 (vehicle(s) [2])"),
        ("speed_plan_params value", lambda: RT.speed_plan_params(B, device="cpu", a_brake=[0.7, 0.0, 0.7]),
         "speed plan rows: a_lat > 0 (+inf: no limit), a_brake > 0 and finite, v_floor >= 0 and finite, end_stop not NaN (vehicle(s) [1])"),
        ("check_plant_rows shape", lambda: VS.check_plant_rows(np.ones((B, 7))), "plant rows: [B,8] (%s), got (3, 7)" % PLANT),
        ("check_road_rows shape", lambda: VS.check_road_rows(np.ones(8)), "road rows: [B,8] (%s, two unused words), got (8,)" % ROAD),
        ("check_fault_rows shape", lambda: VS.check_fault_rows(np.ones((B, 8))), "fault rows: [B,16] (%s, one unused word), got (3, 8)" % FAULT),
        ("check_llc_rows shape", lambda: VS.check_llc_rows(np.ones((B, 9))), "llc rows: [B,8] (%s), got (3, 9)" % LLC),
        ("check_drive_rows shape", lambda: VS.check_drive_rows(np.ones((B, 9))), "drive rows: [B,8] (%s), got (3, 9)" % DRIVE),
        ("check_wander_rows shape", lambda: VS.check_wander_rows(np.ones((B, 8))),
         "wander rows: [B,24] (S0, A, Q of the channels x, y, psi, v, a_long, a_lat, df_offset, free), got (3, 8)"),
        ("check_road_profile shape", lambda: VS.check_road_profile(np.ones((5, 4))),
         "road profile: [n,8] (mu_scale, a_long, a_lat, v_limit, four unused words), got (5, 4)"),
        ("check_speed_plan_rows shape", lambda: RT.check_speed_plan_rows(np.ones((B, 4))),
         "speed plan rows: [B,8] (%s, four unused words), got (3, 4)" % PLAN),
        ("check_road_profile value", lambda: VS.check_road_profile(np.array([[1.0, 0, 0, 1, 0, 0, 0, 0], [0.0, 0, 0, 1, 0, 0, 0, 0]])),
         "road profile: mu_scale must be > 0 and finite (sample(s) [1])"),
    ]
    refused(cases)
    # and what the tables give when nothing is refused: the library's default row, the overrides in their columns, a group in every member
    road = VS.road_params(B, device="cpu", mu=[0.5, 0.6, 0.7], a_lat=1.5).numpy()
    assert (road[:, 0] == road[:, 1]).all() and road[:, 0].tolist() == [0.5, 0.6, 0.7] and (road[:, 3] == 1.5).all() and (road[:, 5] == 1.0).all()
    fault = VS.fault_params(B, device="cpu", win_len=4, p_outlier=[0.0, 0.1, 0.2]).numpy()
    assert (fault[:, 9:12] == 4.0).all() and fault[:, 12].tolist() == [0.0, 0.1, 0.2] and (fault[:, 3:6] == 1.0).all() and np.isinf(fault[:, 14]).all()
    for fn, default in ((VS.plant_params, VS.plant_default), (VS.llc_params, VS.llc_default), (VS.drive_params, VS.drive_default),
                        (RT.speed_plan_params, RT.speed_plan_default), (VS.road_params, VS.road_default), (VS.fault_params, VS.fault_default)):
        assert np.array_equal(fn(B, device="cpu").numpy(), np.tile(default(), (B, 1))), fn.__name__
    assert VS.road_profile_default().tolist() == [1.0, 0.0, 0.0, float("inf"), 0.0, 0.0, 0.0, 0.0] and not VS.wander_default().any()


def test_loop_refusals_of_a_stage_for_another_fleet():
    """the five "X for %d vehicles on %s, plant with %d on %s" texts (and the wander's own), through _ScoredLoop._init_*"""
    import torch
    from mkz_mpc_path_follower_amd.closed_loop import _ScoredLoop
    from mkz_mpc_path_follower_amd.vehicle_sim import DisturbanceObserver, Estimator, LatencyCompensator, SensorModel, Wander, wander_rows

    class Sim:
        B, device, road = B, torch.device("cpu"), None
    loop = _ScoredLoop()
    loop.B, loop.sim, loop.grt = B, Sim(), object()
    far = _ScoredLoop()   # the same stages against a plant on another device: only the device differs
    far.B, far.sim, far.grt = B, types.SimpleNamespace(B=B, device=torch.device("cuda", 0), road=None), loop.grt
    text = "%s for %d vehicles on cpu, plant with 3 on %s"
    planner = lambda n: types.SimpleNamespace(fleet=loop.grt, device=torch.device("cpu"), B=n)
    refused([
        ("sensor B", lambda: loop._init_sensor(SensorModel(4, device="cpu")), text % ("sensor", 4, "cpu")),
        ("sensor device", lambda: far._init_sensor(SensorModel(B, device="cpu")), text % ("sensor", 3, "cuda:0")),
        ("estimator B", lambda: loop._init_estimator(Estimator(4, device="cpu"), "actuator"), text % ("estimator", 4, "cpu")),
        ("estimator device", lambda: far._init_estimator(Estimator(B, device="cpu"), "actuator"), text % ("estimator", 3, "cuda:0")),
        ("observer B", lambda: loop._init_estimator(None, "actuator", None, DisturbanceObserver(4, device="cpu")), text % ("observer", 4, "cpu")),
        ("observer device", lambda: far._init_estimator(None, "command", None, DisturbanceObserver(B, device="cpu")), text % ("observer", 3, "cuda:0")),
        ("compensator B", lambda: loop._init_estimator(None, "history", LatencyCompensator(4, device="cpu")), text % ("compensator", 4, "cpu")),
        ("compensator device", lambda: far._init_estimator(None, "history", LatencyCompensator(B, device="cpu")), text % ("compensator", 3, "cuda:0")),
        ("planner B", lambda: loop._init_planner(planner(4), False), text % ("planner", 4, "cpu")),
        ("planner device", lambda: far._init_planner(planner(B), False), text % ("planner", 3, "cuda:0")),
        ("wander B", lambda: loop._init_wander(Wander(4, wander_rows(4), device="cpu")), "wander= is a vehicle_sim.Wander for 3 vehicles on cpu"),
        ("wander device", lambda: far._init_wander(Wander(B, wander_rows(B), device="cpu")), "wander= is a vehicle_sim.Wander for 3 vehicles on cuda:0"),
        # the order of _init_estimator's checks: the observer's fleet before the compensator's, the compensator's before the estimator's
        ("observer before compensator", lambda: loop._init_estimator(None, "history", LatencyCompensator(4, device="cpu", disturbances=True),
                                                                     DisturbanceObserver(5, device="cpu")), text % ("observer", 5, "cpu")),
        ("compensator before estimator", lambda: loop._init_estimator(Estimator(5, device="cpu"), "history", LatencyCompensator(4, device="cpu")),
         text % ("compensator", 4, "cpu")),
    ])
    sensor = SensorModel(B, device="cpu")
    loop._init_sensor(sensor)
    loop._init_estimator(Estimator(B, device="cpu"), "command")
    assert loop.sensor is sensor and loop.estimator.B == B and loop.compensator is None and loop.observer is None


def test_range_sensor_and_search_contracts():
    """RangeSensor.__init__ / _check and check_search: the radar's rows are a public tensor, checked where it is built and again by every cap()"""
    import torch
    from mkz_mpc_path_follower_amd.ref_traj import RangeSensor, check_search, range_params
    rows = "rows must be a contiguous float64 tensor [3,16] on cpu (range_params; write into it in place)"
    seed = "seed: an integer in 0 ... 2^64 - 1"
    radar = RangeSensor(B, device="cpu")
    refused([
        ("radar seed < 0", lambda: RangeSensor(B, device="cpu", seed=-1), seed),
        ("radar seed 2^64", lambda: RangeSensor(B, device="cpu", seed=2 ** 64), seed),
        ("radar seed before rows", lambda: RangeSensor(B, device="cpu", seed=-1, rows=f64(B, 8)), seed),
        ("radar rows float32", lambda: RangeSensor(B, device="cpu", rows=f64(B, 16).float()), rows),
        ("radar rows for another fleet", lambda: RangeSensor(B, device="cpu", rows=range_params(4, "cpu")), rows),
        ("radar rows follow-sized", lambda: RangeSensor(B, device="cpu", rows=f64(B, 8)), rows),
        ("radar rows strided", lambda: RangeSensor(B, device="cpu", rows=strided(16)), rows),
        ("radar rows numpy", lambda: RangeSensor(B, device="cpu", rows=np.zeros((B, 16))), rows),
        ("radar rows replaced float32", swapped(radar, "rows", radar.rows.float(), radar._check), rows),
        ("radar rows replaced strided", swapped(radar, "rows", strided(16), radar._check), rows),
        ("radar rows replaced numpy", swapped(radar, "rows", radar.rows.numpy(), radar._check), rows),
        ("search unknown", lambda: check_search("fast"), "search= must be one of 'pairs' / 'sorted', got 'fast'"),
        ("search None", lambda: check_search(None), "search= must be one of 'pairs' / 'sorted', got None"),
    ])
    radar._check()
    assert check_search("pairs") == "pairs" and check_search("sorted") == "sorted"
    assert radar.rows.dtype == torch.float64 and radar.rec.shape == (B, 16) and radar.meas.shape == (B, 4)
    assert sorted(radar.summary()) == sorted(("gap_hat", "v_hat", "p00", "p01", "p11", "track_id", "coast", "n", "n_detect", "n_drop", "n_out", "n_new",
                                              "n_lost", "n_bound", "sum_egap2", "max_egap"))
    assert radar.summary()["track_id"].tolist() == [-1, -1, -1] and radar.summary()["track_id"].dtype == np.int64


def test_loop_refusals_of_a_path_stage():
    """_init_planner, _init_follower and _init_lanes: the grid, the stage's own helper, its fleet, the time mode -- in that order, each stage in
    its own sentences (lanes= refuses a follower first)"""
    import torch
    from mkz_mpc_path_follower_amd.closed_loop import _ScoredLoop
    cpu = torch.device("cpu")
    grt = types.SimpleNamespace(time_mode=None)
    timed = types.SimpleNamespace(time_mode=torch.tensor([0, 1, 0], dtype=torch.uint8))
    single = types.SimpleNamespace()   # a one-path helper has no time_mode at all

    def loop(helper, follower=None):
        lp = _ScoredLoop()
        lp.B, lp.grt, lp.follower = B, helper, follower
        lp.sim = types.SimpleNamespace(B=B, device=cpu, road=None)
        return lp
    stage = lambda helper, n=B, **kw: types.SimpleNamespace(fleet=helper, device=cpu, B=n, **kw)
    lanes = lambda helper, n=B: stage(helper, n, shift=None)
    fleet = "%s for %d vehicles on cpu, plant with 3 on cpu"
    mode = "%s= needs every vehicle in target-velocity mode: the fleet helper has vehicles in time mode"
    p_own = "planner= must be a ref_traj.SpeedPlanner built on this loop's own waypoint helper (a FleetRefTrajectory)"
    f_own = "follower= must be a ref_traj.Follower built on this loop's own waypoint helper"
    l_own = "lanes= must be a ref_traj.Lanes built on this loop's own waypoint helper"
    p_grid = "planner= plans a speed along the arclength grid: track_with_time must stay False"
    f_grid = "follower= caps a speed on the arclength grid: track_with_time must stay False"
    l_grid = "lanes= caps a speed on the arclength grid: track_with_time must stay False"
    l_both = "lanes= takes the follower's place (its leaders are found by lane): give no follower="
    refused([
        ("planner grid", lambda: loop(grt)._init_planner(stage(grt), True), p_grid),
        ("planner helper", lambda: loop(grt)._init_planner(stage(timed), False), p_own),
        ("planner no stage at all", lambda: loop(grt)._init_planner(object(), False), p_own),
        ("planner fleet", lambda: loop(grt)._init_planner(stage(grt, 4), False), fleet % ("planner", 4)),
        ("planner mode", lambda: loop(timed)._init_planner(stage(timed), False), mode % "planner"),
        ("planner: the grid before the helper", lambda: loop(grt)._init_planner(stage(timed, 4), True), p_grid),
        ("planner: the helper before the fleet", lambda: loop(grt)._init_planner(stage(timed, 4), False), p_own),
        ("planner: the fleet before the mode", lambda: loop(timed)._init_planner(stage(timed, 4), False), fleet % ("planner", 4)),
        ("follower grid", lambda: loop(grt)._init_follower(stage(grt), True), f_grid),
        ("follower helper", lambda: loop(grt)._init_follower(stage(timed), False), f_own),
        ("follower no stage at all", lambda: loop(grt)._init_follower(object(), False), f_own),
        ("follower fleet", lambda: loop(grt)._init_follower(stage(grt, 5), False), fleet % ("follower", 5)),
        ("follower mode", lambda: loop(timed)._init_follower(stage(timed), False), mode % "follower"),
        ("follower: the grid before the helper", lambda: loop(grt)._init_follower(stage(timed, 4), True), f_grid),
        ("follower: the helper before the fleet", lambda: loop(grt)._init_follower(stage(timed, 4), False), f_own),
        ("follower: the fleet before the mode", lambda: loop(timed)._init_follower(stage(timed, 4), False), fleet % ("follower", 4)),
        ("lanes with a follower", lambda: loop(grt, stage(grt))._init_lanes(lanes(grt), False), l_both),
        ("lanes grid", lambda: loop(grt)._init_lanes(lanes(grt), True), l_grid),
        ("lanes helper", lambda: loop(grt)._init_lanes(lanes(timed), False), l_own),
        ("lanes a follower in their place", lambda: loop(grt)._init_lanes(stage(grt), False), l_own),
        ("lanes fleet", lambda: loop(grt)._init_lanes(lanes(grt, 2), False), fleet % ("lanes", 2)),
        ("lanes mode", lambda: loop(timed)._init_lanes(lanes(timed), False), mode % "lanes"),
        ("lanes: the follower before the grid", lambda: loop(grt, stage(grt))._init_lanes(lanes(timed, 4), True), l_both),
        ("lanes: the grid before the helper", lambda: loop(grt)._init_lanes(lanes(timed, 4), True), l_grid),
        ("lanes: the helper before the fleet", lambda: loop(grt)._init_lanes(lanes(timed, 4), False), l_own),
        ("lanes: the fleet before the mode", lambda: loop(timed)._init_lanes(lanes(timed, 4), False), fleet % ("lanes", 4)),
    ])
    lp = loop(single)   # a one-path helper (no time_mode) passes the follower's and the lanes' mode check; nothing given is nothing checked
    fol, ln = stage(single), lanes(single)
    lp._init_follower(fol, False)
    assert lp.follower is fol and lp.v_follow is None
    lp.follower = None
    lp._init_lanes(ln, False)
    assert lp.lanes is ln
    lp = loop(grt)
    lp._init_planner(None, True), lp._init_follower(None, True), lp._init_lanes(None, True)
    assert lp.planner is None and lp.v_plan is None and lp.follower is None and lp.lanes is None


# ---- what needs a device to construct -------------------------------------------------------------------------------------
def _fleet():
    import fleet_scenario as F
    from mkz_mpc_path_follower_amd import FleetRefTrajectory
    return FleetRefTrajectory([F.path_dict(0), F.path_dict(1)], [0, 1, 0], time_mode=[0, 0, 0], traj_horizon=8, traj_dt=0.2)


@pytest.mark.gpu
def test_simulator_tensors_must_stay():
    """VehicleSimulator._update_vehicle_model after a public tensor was replaced: refused before the launch (no road profile here: its launch comes
    before the drive rows are looked at)"""
    import torch
    from mkz_mpc_path_follower_amd.vehicle_sim import SensorModel, VehicleSimulator, drive_params, fault_params, road_params
    sim = VehicleSimulator(B, road=road_params(B), drive=drive_params(B), cmd_queue_depth=3, cmd_delay=2)
    held = VehicleSimulator(B, cmd_delay=2)
    step = sim._update_vehicle_model
    base = "state [B,8] / cmd [B,2] must stay contiguous float64 tensors on cuda:0 (write into them with copy_)"
    queue = "plant [B,8] / cmd_queue [D,B,2] float64 and cmd_delay [B] int32 must stay contiguous tensors on cuda:0 (write into them with copy_)"
    road = "road [B,8] / road_stat [B,4] must stay contiguous float64 tensors on cuda:0 (write into them with copy_)"
    drive = "drive [B,8] must stay a contiguous float64 tensor on cuda:0 (write into it with copy_)"
    llc = "params [B,8] and rec [B,16] must stay contiguous float64 tensors on cuda:0 (write into them with copy_)"
    plant = "plant [B,8] / cmd_held [B,2] float64 and cmd_delay [B] int32 must stay contiguous tensors on cuda:0 (write into them with copy_)"
    t = lambda x: x.t().contiguous().t()   # the same shape and values, not contiguous
    sen = SensorModel(B, meas_delay=1, faults=fault_params(B))
    ring = SensorModel(B, meas_delay=1)
    state = torch.zeros((B, 8), dtype=torch.float64, device=sim.device)
    faults = ("faults / fault_record [B,16] and z [B,4] float64, flags [B] int32, blind [B] uint8, meas_delay [B] int32 and truth_ring [depth,B,4] float64 "
              "must stay contiguous tensors on cuda:0")
    refused([
        ("state float32", swapped(sim, "state", sim.state.float(), step), base),
        ("cmd transposed", swapped(sim, "cmd", t(sim.cmd), step), base),
        ("plant float32", swapped(sim, "plant", sim.plant.float(), step), queue),
        ("plant transposed", swapped(sim, "plant", t(sim.plant), step), queue),
        ("plant numpy", swapped(sim, "plant", np.zeros((B, 8)), step), queue),
        ("cmd_queue float32", swapped(sim, "cmd_queue", sim.cmd_queue.float(), step), queue),
        ("cmd_queue transposed", swapped(sim, "cmd_queue", sim.cmd_queue.transpose(0, 1), step), queue),
        ("cmd_delay int64", swapped(sim, "cmd_delay", sim.cmd_delay.long(), step), queue),
        ("road float32", swapped(sim, "road", sim.road.float(), step), road),
        ("road transposed", swapped(sim, "road", t(sim.road), step), road),
        ("road_stat on the host", swapped(sim, "road_stat", sim.road_stat.cpu(), step), road),
        ("drive float32", swapped(sim, "drive", sim.drive.float(), step), drive),
        ("drive transposed", swapped(sim, "drive", t(sim.drive), step), drive),
        ("llc rec float32", swapped(sim.llc, "rec", sim.llc.rec.float(), step), llc),
        ("cmd_held float32", swapped(held, "cmd_held", held.cmd_held.float(), held._update_vehicle_model), plant),
        ("held plant transposed", swapped(held, "plant", t(held.plant), held._update_vehicle_model), plant),
        ("sensor flags int64", swapped(sen, "flags", sen.flags.long(), lambda: sen.sense(state, 0)), faults),
        ("sensor faults float32", swapped(sen, "faults", sen.faults.float(), lambda: sen.sense(state, 0)), faults),
        ("sensor ring transposed", swapped(ring, "truth_ring", ring.truth_ring.transpose(0, 1), lambda: ring.sense(state, 0)),
         "meas_delay [B] int32 and truth_ring [depth,B,4] float64 must stay contiguous tensors on cuda:0"),
    ])
    assert sim.period == 0 and sim.plant.dtype == torch.float64 and sim.plant.is_contiguous()


@pytest.mark.gpu
def test_fleet_profile_and_planner_contracts():
    """RoadProfile.apply, SpeedPlanner.plan(out=...) and _check_rows, and the fleet helper's `path_id` / `time_mode` "must stay" refusals"""
    import torch
    from mkz_mpc_path_follower_amd.ref_traj import SpeedPlanner, fresh_score
    from mkz_mpc_path_follower_amd.vehicle_sim import RoadProfile
    grt = _fleet()
    dev = grt.device
    prof, pl = RoadProfile(grt), SpeedPlanner(grt)
    d64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
    state, rows, out, vcap = d64(B, 8), d64(B, 8), d64(B, 8), d64(B)
    pose = d64(B, 3)
    pid = "path_id must stay a contiguous int32 tensor [3] on cuda:0 (write into it in place)"
    st = "state: a float64 tensor [3,W] on cuda:0 with X, Y in the first two columns"
    row = "%s: a contiguous float64 tensor [3,8] on cuda:0"
    table = "table must stay a contiguous float64 tensor [%d,8] on cuda:0 (write into it with copy_)" % prof.total
    prows = "rows must be a contiguous float64 tensor [3,8] on cuda:0 (speed_plan_params; write into it in place)"
    pout = "out: expected a contiguous float64 tensor [3] on cuda:0"
    buf = "%s: expected a contiguous %s tensor %s on cuda:0"
    good = dict(status=torch.zeros(B, dtype=torch.int32, device=dev), iters=torch.zeros(B, dtype=torch.int32, device=dev), cmd=d64(B, 2),
                stop_latch=torch.zeros(B, dtype=torch.bool, device=dev))
    score = lambda **kw: grt.track_score_batch(state, score=fresh_score(B, dev), **dict(good, **kw))
    refused([
        ("profile table float32", swapped(prof, "table", prof.table.float(), lambda: prof.apply(state, rows, out)), table),
        ("profile table numpy", swapped(prof, "table", np.zeros((prof.total, 8)), lambda: prof.apply(state, rows, out)), table),
        ("apply state float32", lambda: prof.apply(state.float(), rows, out), st),
        ("apply state one column", lambda: prof.apply(d64(B, 1), rows, out), st),
        ("apply state transposed", lambda: prof.apply(d64(8, B).t(), rows, out), st),
        ("apply state numpy", lambda: prof.apply(np.zeros((B, 8)), rows, out), st),
        ("apply road_base float32", lambda: prof.apply(state, rows.float(), out), row % "road_base"),
        ("apply out shape", lambda: prof.apply(state, rows, d64(B, 6)), row % "out"),
        ("apply out transposed", lambda: prof.apply(state, rows, d64(8, B).t()), row % "out"),
        ("apply path_id int64", swapped(grt, "path_id", grt.path_id.long(), lambda: prof.apply(state, rows, out)), pid),
        ("plan out float32", lambda: pl.plan(state, vcap, out=vcap.float()), pout),
        ("plan out shape", lambda: pl.plan(state, vcap, out=d64(B, 1)), pout),
        ("plan out strided", lambda: pl.plan(state, vcap, out=d64(2 * B)[::2]), pout),
        ("plan out numpy", lambda: pl.plan(state, vcap, out=np.zeros(B)), pout),
        ("plan rows float32", swapped(pl, "rows", pl.rows.float(), lambda: pl.plan(state, vcap)), prows),
        ("plan rows transposed", swapped(pl, "rows", d64(8, B).t(), pl._check_rows), prows),
        ("plan rows numpy", swapped(pl, "rows", np.zeros((B, 8)), pl._check_rows), prows),
        ("plan path_id int64", swapped(grt, "path_id", grt.path_id.long(), lambda: pl.plan(state, vcap)), pid),
        ("plan v_cap shape", lambda: pl.plan(state, d64(B + 1)), "v_cap: expected [3], got (4,)"),
        ("waypoints path_id int64", swapped(grt, "path_id", grt.path_id.long(), lambda: grt.get_waypoints_batch(pose, vcap)), pid),
        ("waypoints path_id strided", swapped(grt, "path_id", torch.zeros(2 * B, dtype=torch.int32, device=dev)[::2],
                                              lambda: grt.get_waypoints_batch(pose, vcap)), pid),
        ("waypoints time_mode bool", swapped(grt, "time_mode", grt.time_mode.bool(), lambda: grt.get_waypoints_batch(pose, vcap)),
         "time_mode must stay a contiguous uint8 tensor [3] on cuda:0 (write into it in place)"),
        ("waypoints time_mode on the host", swapped(grt, "time_mode", grt.time_mode.cpu(), lambda: grt.get_waypoints_batch(pose, vcap)),
         "time_mode must stay a contiguous uint8 tensor [3] on cuda:0 (write into it in place)"),
        ("score path_id int64", swapped(grt, "path_id", grt.path_id.long(), lambda: grt.track_score_batch(state)), pid),
        ("score status int64", lambda: score(status=good["status"].long()), buf % ("status", "torch.int32", "(3,)")),
        ("score cmd shape", lambda: score(cmd=d64(B, 3)), buf % ("cmd", "torch.float64", "(3, 2)")),
        ("score latch int32", lambda: score(stop_latch=good["status"]), buf % ("stop_latch", "torch.uint8", "(3,)")),
        ("score record float32", lambda: grt.track_score_batch(state, score=d64(B, 16).float()), buf % ("score", "torch.float64", "(3, 16)")),
        ("score out err strided", lambda: grt.track_score_batch(state, out=dict(err=d64(4, B).t())), buf % ("err", "torch.float64", "(3, 4)")),
    ])
    assert grt.path_id.dtype == torch.int32 and grt.time_mode.dtype == torch.uint8 and pl.rows.dtype == torch.float64


def _single():
    import fleet_scenario as F
    from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory
    d = F.path_dict(0)
    return GPSRefTrajectory(arrays=d, traj_horizon=8, traj_dt=0.2, lat0=d["lat0"], lon0=d["lon0"])


@pytest.mark.gpu
def test_planner_state_contracts():
    """SpeedPlanner.plan's state: the plant's state or a view of it passes as it is, anything else is copied first and then refused by shape"""
    import torch
    from mkz_mpc_path_follower_amd.ref_traj import SpeedPlanner
    grt = _fleet()
    dev = grt.device
    pl = SpeedPlanner(grt)
    d64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
    st = "state: expected [3,W] with X, Y in the first two columns, got %s"
    refused([
        ("plan state one column", lambda: pl.plan(d64(B, 1), d64(B)), st % "(3, 1)"),
        ("plan state rows", lambda: pl.plan(d64(B + 1, 8), d64(B)), st % "(4, 8)"),
        ("plan state 1-D", lambda: pl.plan(d64(B), d64(B)), st % "(3,)"),
        ("plan state numpy rows", lambda: pl.plan(np.zeros((2, 8)), d64(B)), st % "(2, 8)"),
        ("plan state float32 one column", lambda: pl.plan(d64(B, 1).float(), d64(B)), st % "(3, 1)"),
        ("plan v_cap shape", lambda: pl.plan(d64(B, 8), d64(B, 1)), "v_cap: expected [3], got (3, 1)"),
        ("plan v_cap numpy length", lambda: pl.plan(d64(B, 8), np.zeros(2)), "v_cap: expected [3], got (2,)"),
        ("plan: the state before v_cap", lambda: pl.plan(d64(B, 1), d64(B + 1)), st % "(3, 1)"),
        ("plan: v_cap before the rows", swapped(pl, "rows", pl.rows.float(), lambda: pl.plan(d64(B, 8), d64(B + 1))), "v_cap: expected [3], got (4,)"),
        ("plan: the rows before path_id", swapped(grt, "path_id", grt.path_id.long(), swapped(pl, "rows", pl.rows.float(), lambda: pl.plan(d64(B, 8), d64(B)))),
         "rows must be a contiguous float64 tensor [3,8] on cuda:0 (speed_plan_params; write into it in place)"),
        ("plan: path_id before out", swapped(grt, "path_id", grt.path_id.long(), lambda: pl.plan(d64(B, 8), d64(B), out=d64(B + 1))),
         "path_id must stay a contiguous int32 tensor [3] on cuda:0 (write into it in place)"),
    ])


@pytest.mark.gpu
def test_follower_contracts():
    """Follower.__init__ / cap / gap_seen, without and with a radar: every refusal, and the order of cap()'s checks"""
    import torch
    from mkz_mpc_path_follower_amd.ref_traj import Follower, RangeSensor, follow_params
    grt = _fleet()
    dev = grt.device
    d64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
    u8 = lambda n: torch.ones(n, dtype=torch.uint8, device=dev)
    fol = Follower(grt)
    rad = Follower(grt, radar=RangeSensor(B, dev))
    state, vcap = d64(B, 8), d64(B)
    rows = "rows must be a contiguous float64 tensor [3,8] on cuda:0 (follow_params; write into it in place)"
    radar = "radar= must be a ref_traj.RangeSensor for 3 vehicles on cuda:0"
    none = "known=, k= and dt= are read by a radar: this Follower has none (radar=RangeSensor(...))"
    need = "a Follower with a radar needs the period's index k= (the draws' counter) and its length dt= [s] in every cap()"
    st = "state: expected [3,W] with X, Y, psi, v in the first four columns, got %s"
    kn = "known: expected [3,W] with v in column 3, got %s"
    pid = "path_id must stay a contiguous int32 tensor [3] on cuda:0 (write into it in place)"
    pres = "present: expected a contiguous uint8 or bool tensor [3] on cuda:0"
    stat = "stat must stay a contiguous float64 tensor [3,8] on cuda:0 (reset() gives a fresh one)"
    out = "out: expected a contiguous float64 tensor [3] on cuda:0"
    rrows = "rows must be a contiguous float64 tensor [3,16] on cuda:0 (range_params; write into it in place)"
    rrec = "radar.rec must stay a contiguous float64 tensor [3,16] on cuda:0 (reset() gives a fresh one)"
    seen = "gap_seen and v_lead_seen are a radar's: this Follower has none (radar=RangeSensor(...))"
    cap = lambda **kw: rad.cap(state, vcap, **dict(dict(k=0, dt=0.1), **kw))
    refused([
        ("follower helper", lambda: Follower(object()), "Follower follows on a GPSRefTrajectory or a FleetRefTrajectory; a object is neither"),
        ("follower one path without rows", lambda: Follower(_single()),
         "Follower on a GPSRefTrajectory: rows [B,8] (follow_params) are required, their length is the fleet's size"),
        ("follower one path numpy rows", lambda: Follower(_single(), rows=np.zeros((B, 8))),
         "Follower on a GPSRefTrajectory: rows [B,8] (follow_params) are required, their length is the fleet's size"),
        ("follower rows float32", lambda: Follower(grt, rows=d64(B, 8).float()), rows),
        ("follower rows for another fleet", lambda: Follower(grt, rows=follow_params(4, dev)), rows),
        ("follower rows strided", lambda: Follower(grt, rows=d64(8, B).t()), rows),
        ("follower rows numpy", lambda: Follower(grt, rows=np.zeros((B, 8))), rows),
        ("follower rows on the host", lambda: Follower(grt, rows=follow_params(B, "cpu")), rows),
        ("follower radar for another fleet", lambda: Follower(grt, radar=RangeSensor(4, dev)), radar),
        ("follower radar on the host", lambda: Follower(grt, radar=RangeSensor(B, "cpu")), radar),
        ("follower radar no sensor", lambda: Follower(grt, radar=object()), radar),
        ("follower search", lambda: Follower(grt, search="tree"), "search= must be one of 'pairs' / 'sorted', got 'tree'"),
        ("follower: the rows before the radar", lambda: Follower(grt, rows=d64(B, 8).float(), radar=object()), rows),
        ("follower: the radar before the search", lambda: Follower(grt, radar=object(), search="tree"), radar),
        ("gap_seen without a radar", lambda: fol.gap_seen, seen),
        ("v_lead_seen without a radar", lambda: fol.v_lead_seen, seen),
        ("cap known without a radar", lambda: fol.cap(state, vcap, known=state), none),
        ("cap k without a radar", lambda: fol.cap(state, vcap, k=0), none),
        ("cap dt without a radar", lambda: fol.cap(state, vcap, dt=0.1), none),
        ("cap state three columns", lambda: fol.cap(d64(B, 3), vcap), st % "(3, 3)"),
        ("cap state rows", lambda: fol.cap(d64(B + 1, 8), vcap), st % "(4, 8)"),
        ("cap state numpy rows", lambda: fol.cap(np.zeros((2, 8)), vcap), st % "(2, 8)"),
        ("cap state float32 three columns", lambda: fol.cap(d64(B, 3).float(), vcap), st % "(3, 3)"),
        ("cap state 1-D", lambda: fol.cap(d64(B), vcap), st % "(3,)"),
        ("cap v_cap shape", lambda: fol.cap(state, d64(B + 1)), "v_cap: expected [3], got (4,)"),
        ("cap v_cap column", lambda: fol.cap(state, d64(B, 1)), "v_cap: expected [3], got (3, 1)"),
        ("cap rows float32", swapped(fol, "rows", fol.rows.float(), lambda: fol.cap(state, vcap)), rows),
        ("cap rows strided", swapped(fol, "rows", d64(8, B).t(), lambda: fol.cap(state, vcap)), rows),
        ("cap rows numpy", swapped(fol, "rows", np.zeros((B, 8)), lambda: fol.cap(state, vcap)), rows),
        ("cap path_id int64", swapped(grt, "path_id", grt.path_id.long(), lambda: fol.cap(state, vcap)), pid),
        ("cap path_id strided", swapped(grt, "path_id", torch.zeros(2 * B, dtype=torch.int32, device=dev)[::2], lambda: fol.cap(state, vcap)), pid),
        ("cap path_id numpy", swapped(grt, "path_id", np.zeros(B, dtype=np.int32), lambda: fol.cap(state, vcap)), pid),
        ("cap present int32", lambda: fol.cap(state, vcap, present=torch.ones(B, dtype=torch.int32, device=dev)), pres),
        ("cap present length", lambda: fol.cap(state, vcap, present=u8(B + 1)), pres),
        ("cap present strided", lambda: fol.cap(state, vcap, present=u8(2 * B)[::2]), pres),
        ("cap present numpy", lambda: fol.cap(state, vcap, present=np.ones(B, dtype=np.uint8)), pres),
        ("cap stat float32", swapped(fol, "stat", fol.stat.float(), lambda: fol.cap(state, vcap)), stat),
        ("cap stat strided", swapped(fol, "stat", d64(8, B).t(), lambda: fol.cap(state, vcap)), stat),
        ("cap stat numpy", swapped(fol, "stat", np.zeros((B, 8)), lambda: fol.cap(state, vcap)), stat),
        ("cap out float32", lambda: fol.cap(state, vcap, out=vcap.float()), out),
        ("cap out shape", lambda: fol.cap(state, vcap, out=d64(B, 1)), out),
        ("cap out strided", lambda: fol.cap(state, vcap, out=d64(2 * B)[::2]), out),
        ("cap out numpy", lambda: fol.cap(state, vcap, out=np.zeros(B)), out),
        ("cap: the state before v_cap", lambda: fol.cap(d64(B, 3), d64(B + 1)), st % "(3, 3)"),
        ("cap: v_cap before the rows", swapped(fol, "rows", fol.rows.float(), lambda: fol.cap(state, d64(B + 1))), "v_cap: expected [3], got (4,)"),
        ("cap: the rows before path_id", swapped(grt, "path_id", grt.path_id.long(), swapped(fol, "rows", fol.rows.float(), lambda: fol.cap(state, vcap))), rows),
        ("cap: path_id before present", swapped(grt, "path_id", grt.path_id.long(), lambda: fol.cap(state, vcap, present=u8(B + 1))), pid),
        ("cap: present before stat", swapped(fol, "stat", fol.stat.float(), lambda: fol.cap(state, vcap, present=u8(B + 1))), pres),
        ("cap: stat before out", swapped(fol, "stat", fol.stat.float(), lambda: fol.cap(state, vcap, out=d64(B + 1))), stat),
        ("radar cap without k", lambda: rad.cap(state, vcap, dt=0.1), need),
        ("radar cap without dt", lambda: rad.cap(state, vcap, k=0), need),
        ("radar cap k < 0", lambda: cap(k=-1), "k >= 0 and a finite dt > 0, got k=-1, dt=0.1"),
        ("radar cap dt 0", lambda: cap(dt=0), "k >= 0 and a finite dt > 0, got k=0, dt=0.0"),
        ("radar cap dt inf", lambda: cap(k=2, dt=float("inf")), "k >= 0 and a finite dt > 0, got k=2, dt=inf"),
        ("radar cap known three columns", lambda: cap(known=d64(B, 3)), kn % "(3, 3)"),
        ("radar cap known rows", lambda: cap(known=d64(B + 1, 4)), kn % "(4, 4)"),
        ("radar cap known numpy rows", lambda: cap(known=np.zeros((2, 4))), kn % "(2, 4)"),
        ("radar cap known float32 three columns", lambda: cap(known=d64(B, 3).float()), kn % "(3, 3)"),
        ("radar cap state as known", lambda: rad.cap(d64(B, 3), vcap, k=0, dt=0.1), kn % "(3, 3)"),
        ("radar rows float32", swapped(rad.radar, "rows", rad.radar.rows.float(), cap), rrows),
        ("radar rows strided", swapped(rad.radar, "rows", d64(16, B).t(), cap), rrows),
        ("radar rows numpy", swapped(rad.radar, "rows", np.zeros((B, 16)), cap), rrows),
        ("radar rec float32", swapped(rad.radar, "rec", rad.radar.rec.float(), cap), rrec),
        ("radar rec strided", swapped(rad.radar, "rec", d64(16, B).t(), cap), rrec),
        ("radar rec numpy", swapped(rad.radar, "rec", np.zeros((B, 16)), cap), rrec),
        ("radar: k and dt before known", lambda: cap(k=-1, known=d64(B, 3)), "k >= 0 and a finite dt > 0, got k=-1, dt=0.1"),
        ("radar: known before the radar's rows", swapped(rad.radar, "rows", rad.radar.rows.float(), lambda: cap(known=d64(B, 3))), kn % "(3, 3)"),
        ("radar: the radar's rows before its rec", swapped(rad.radar, "rec", rad.radar.rec.float(), swapped(rad.radar, "rows", rad.radar.rows.float(), cap)), rrows),
        ("radar: the radar's rec before the state", swapped(rad.radar, "rec", rad.radar.rec.float(), lambda: rad.cap(d64(B, 3), vcap, known=state, k=0, dt=0.1)), rrec),
        ("radar: the state before v_cap", lambda: rad.cap(d64(B, 3), d64(B + 1), known=state, k=0, dt=0.1), st % "(3, 3)"),
    ])
    assert grt.path_id.dtype == torch.int32 and fol.rows.dtype == torch.float64 and fol.stat.dtype == torch.float64
    assert rad.radar.rows.dtype == torch.float64 and rad.radar.rec.dtype == torch.float64
    assert rad.gap_seen.tolist() == [float("inf")] * B and rad.v_lead_seen.tolist() == [0.0] * B   # no track yet
    assert fol.gap.tolist() == [float("inf")] * B and fol.leader_speed.tolist() == [0.0] * B and fol.leader.tolist() == [-1] * B


@pytest.mark.gpu
def test_lanes_contracts():
    """Lanes.__init__ / step / shift: every refusal, and the order of step()'s checks"""
    import torch
    from mkz_mpc_path_follower_amd.ref_traj import Lanes, follow_params, lane_params
    grt = _fleet()
    dev = grt.device
    d64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
    u8 = lambda n: torch.ones(n, dtype=torch.uint8, device=dev)
    ln = Lanes(grt, lane_rows=lane_params(B, dev, n_lanes=2))
    state, vcap, ref = d64(B, 8), d64(B), d64(B, 9, 3)
    rows = "rows must be a contiguous float64 tensor [3,8] on cuda:0 (lane_params; write into it in place)"
    frows = "follow_rows must be a contiguous float64 tensor [3,8] on cuda:0 (follow_params; write into it in place)"
    one = "Lanes on a GPSRefTrajectory: rows [B,8] (follow_params or lane_params) are required, their length is the fleet's size"
    lane0 = "lane0: one integer lane per vehicle [3], each inside 0 ... n_lanes - 1 of its lane row"
    st = "state: expected [3,W] with X, Y, psi, v in the first four columns, got %s"
    pid = "path_id must stay a contiguous int32 tensor [3] on cuda:0 (write into it in place)"
    pres = "present: expected a contiguous uint8 or bool tensor [3] on cuda:0"
    rec = "rec must stay a contiguous float64 tensor [3,16] on cuda:0 (reset() gives a fresh one)"
    out = "out: expected a contiguous float64 tensor [3] on cuda:0"
    rtext = "ref: expected a contiguous float64 tensor [3,H+1,3] on cuda:0"
    step = lambda s=state, v=vcap, **kw: ln.step(s, v, 0, 0.1, **kw)
    refused([
        ("lanes helper", lambda: Lanes(object()), "Lanes run on a GPSRefTrajectory or a FleetRefTrajectory; a object is neither"),
        ("lanes one path without rows", lambda: Lanes(_single()), one),
        ("lanes one path numpy rows", lambda: Lanes(_single(), follow_rows=np.zeros((B, 8)), lane_rows=np.zeros((B, 8))), one),
        ("lanes rows float32", lambda: Lanes(grt, lane_rows=d64(B, 8).float()), rows),
        ("lanes rows for another fleet", lambda: Lanes(grt, lane_rows=lane_params(4, dev)), rows),
        ("lanes rows strided", lambda: Lanes(grt, lane_rows=d64(8, B).t()), rows),
        ("lanes rows numpy", lambda: Lanes(grt, lane_rows=np.zeros((B, 8))), rows),
        ("lanes follow_rows float32", lambda: Lanes(grt, follow_rows=d64(B, 8).float()), frows),
        ("lanes follow_rows for another fleet", lambda: Lanes(grt, follow_rows=follow_params(4, dev)), frows),
        ("lanes follow_rows numpy", lambda: Lanes(grt, follow_rows=np.zeros((B, 8))), frows),
        ("lanes: the lane rows before the follow rows", lambda: Lanes(grt, follow_rows=d64(B, 8).float(), lane_rows=d64(B, 8).float()), rows),
        ("lanes lane0 length", lambda: Lanes(grt, lane0=[0, 0]), lane0),
        ("lanes lane0 outside", lambda: Lanes(grt, lane0=[0, 1, 0]), lane0),
        ("lanes lane0 fraction", lambda: Lanes(grt, lane_rows=lane_params(B, dev, n_lanes=2), lane0=[0, 0.5, 1]), lane0),
        ("lanes lane0 negative", lambda: Lanes(grt, lane0=torch.tensor([0, -1, 0])), lane0),
        ("lanes search", lambda: Lanes(grt, search="tree"), "search= must be one of 'pairs' / 'sorted', got 'tree'"),
        ("lanes lanes_max 33", lambda: Lanes(grt, search="sorted", lanes_max=33), "lanes_max: an integer in 0 ... 32 or None, got 33"),
        ("lanes lanes_max < 0", lambda: Lanes(grt, search="sorted", lanes_max=-1), "lanes_max: an integer in 0 ... 32 or None, got -1"),
        ("lanes lanes_max float", lambda: Lanes(grt, search="sorted", lanes_max=2.0), "lanes_max: an integer in 0 ... 32 or None, got 2.0"),
        ("lanes lanes_max with pairs", lambda: Lanes(grt, lanes_max=2), "lanes_max= sizes the tables of search=\"sorted\"; the pair search has none"),
        ("lanes: lane0 before the search", lambda: Lanes(grt, lane0=[0, 0], search="tree"), lane0),
        ("step state three columns", lambda: step(d64(B, 3)), st % "(3, 3)"),
        ("step state rows", lambda: step(d64(B + 1, 8)), st % "(4, 8)"),
        ("step state numpy rows", lambda: step(np.zeros((2, 8))), st % "(2, 8)"),
        ("step state float32 three columns", lambda: step(d64(B, 3).float()), st % "(3, 3)"),
        ("step v_cap shape", lambda: step(v=d64(B + 1)), "v_cap: expected [3], got (4,)"),
        ("step rows float32", swapped(ln, "rows", ln.rows.float(), step), rows),
        ("step rows strided", swapped(ln, "rows", d64(8, B).t(), step), rows),
        ("step rows numpy", swapped(ln, "rows", np.zeros((B, 8)), step), rows),
        ("step follow_rows float32", swapped(ln, "follow_rows", ln.follow_rows.float(), step), frows),
        ("step follow_rows strided", swapped(ln, "follow_rows", d64(8, B).t(), step), frows),
        ("step follow_rows numpy", swapped(ln, "follow_rows", np.zeros((B, 8)), step), frows),
        ("step path_id int64", swapped(grt, "path_id", grt.path_id.long(), step), pid),
        ("step path_id strided", swapped(grt, "path_id", torch.zeros(2 * B, dtype=torch.int32, device=dev)[::2], step), pid),
        ("step path_id numpy", swapped(grt, "path_id", np.zeros(B, dtype=np.int32), step), pid),
        ("step present int32", lambda: step(present=torch.ones(B, dtype=torch.int32, device=dev)), pres),
        ("step present length", lambda: step(present=u8(B + 1)), pres),
        ("step present numpy", lambda: step(present=np.ones(B, dtype=np.uint8)), pres),
        ("step rec float32", swapped(ln, "rec", ln.rec.float(), step), rec),
        ("step rec strided", swapped(ln, "rec", d64(16, B).t(), step), rec),
        ("step rec numpy", swapped(ln, "rec", np.zeros((B, 16)), step), rec),
        ("step out float32", lambda: step(out=vcap.float()), out),
        ("step out shape", lambda: step(out=d64(B, 1)), out),
        ("step out strided", lambda: step(out=d64(2 * B)[::2]), out),
        ("step out numpy", lambda: step(out=np.zeros(B)), out),
        ("step: the state before v_cap", lambda: step(d64(B, 3), d64(B + 1)), st % "(3, 3)"),
        ("step: v_cap before the rows", swapped(ln, "rows", ln.rows.float(), lambda: step(v=d64(B + 1))), "v_cap: expected [3], got (4,)"),
        ("step: the rows before path_id", swapped(grt, "path_id", grt.path_id.long(), swapped(ln, "follow_rows", ln.follow_rows.float(), step)), frows),
        ("step: path_id before present", swapped(grt, "path_id", grt.path_id.long(), lambda: step(present=u8(B + 1))), pid),
        ("step: present before rec", swapped(ln, "rec", ln.rec.float(), lambda: step(present=u8(B + 1))), pres),
        ("step: rec before out", swapped(ln, "rec", ln.rec.float(), lambda: step(out=d64(B + 1))), rec),
        ("shift ref float32", lambda: ln.shift(ref.float()), rtext),
        ("shift ref rows", lambda: ln.shift(d64(B + 1, 9, 3)), rtext),
        ("shift ref two words", lambda: ln.shift(d64(B, 9, 2)), rtext),
        ("shift ref 2-D", lambda: ln.shift(d64(B, 3)), rtext),
        ("shift ref strided", lambda: ln.shift(d64(9, B, 3).transpose(0, 1)), rtext),
        ("shift ref numpy", lambda: ln.shift(np.zeros((B, 9, 3))), rtext),
        ("shift rec float32", swapped(ln, "rec", ln.rec.float(), lambda: ln.shift(ref)), rec),
        ("shift rec numpy", swapped(ln, "rec", np.zeros((B, 16)), lambda: ln.shift(ref)), rec),
        ("shift: the ref before rec", swapped(ln, "rec", ln.rec.float(), lambda: ln.shift(ref.float())), rtext),
    ])
    assert grt.path_id.dtype == torch.int32 and ln.rows.dtype == torch.float64 and ln.follow_rows.dtype == torch.float64 and ln.rec.dtype == torch.float64
    assert ln.lane.tolist() == [0.0] * B and ln.offset.tolist() == [0.0] * B and ln.gap.tolist() == [float("inf")] * B
    assert ln.leader_speed.tolist() == [0.0] * B and ln.leader.tolist() == [-1] * B and ln.shift(d64(B, 0, 3)).shape == (B, 0, 3)
