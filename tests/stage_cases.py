"""The cases of tests/golden/stage_kernels_parent.npz (test helper): inputs and drivers shared by tools/record_stage_golden.py, which ran them on the
build BEFORE the stage kernels were given one sub-step and one set of helpers, and tests/test_stage_parent.py, which replays them on the build
under test and requires the same bits.

Every batch has B = 70 vehicles: one full wave and a six-lane tail, so the plant's wave-uniform `__any` branches see a clean wave and a mixed one.
Inputs are functions of the lane index built from +, -, *, / and % alone (IEEE basic operations: the same bits on every host), so the file need not
carry them; it carries one digest of each case's inputs instead and the replay checks that it feeds what the recorder fed.
Outputs: 70 lanes x 8 words x 3 periods x 32 plant runs alone would be 430 KB, so a kernel case keeps one 64-bit FNV-1a digest per lane over the raw
64-bit patterns of everything the case's calls wrote, in call order (any changed bit of any word changes the lane's digest; NaNs count as their
bits).  The two closed loops (8 vehicles, 5 periods) are kept in full."""
import ctypes as C

import numpy as np

B = 70
FNV = np.uint64(0x100000001B3)


def digest(h, a):
    """fold a [B, ...] (float64 as its bits; integers and bools by value) into the per-lane digests h [B] uint64"""
    a = np.ascontiguousarray(a)
    w = (a.view(np.uint64) if a.dtype == np.float64 else a.astype(np.int64).view(np.uint64)).reshape(a.shape[0], -1)
    for k in range(w.shape[1]):
        h = (h ^ w[:, k]) * FNV
    return h


def fresh(n=B):
    return np.full(n, 0xCBF29CE484222325, dtype=np.uint64)


def fold(h):
    """the lanes' digests -> one [1]: what the file keeps of a case's inputs"""
    return digest(fresh(1), h[None, :])


def frac(a, m, k=0):
    """a spread of [0, 1) over the lanes: ((i + k) a mod m) / m"""
    return (((np.arange(B) + k) * a) % m) / float(m)


def sym(a, m, k=0):
    return frac(a, m, k) - 0.5


def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to("cuda:0")


def host(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------- plant kernels
OUTLIERS_TAIL = (64, 65, 66, 67, 68, 69)      # wave 0 stays inside every polynomial's range
OUTLIERS_WAVE0 = (3, 11, 22, 37, 45, 58)      # scattered through wave 0
DEPTH = 3
ROADS = {"neutral": (np.inf, np.inf, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0), "nolimit": (np.inf, np.inf, -0.5, 1.5, 0.02, 0.9, 0.0, 0.0),
         "front": (0.2, np.inf, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0), "both": (0.2, 0.2, -0.5, 1.5, 0.02, 0.9, 0.0, 0.0)}


def plant_inputs(n, outliers):
    s = np.zeros((B, 8))
    s[:, 0] = -300.0 + 1.5 * np.arange(B); s[:, 1] = -450.0 + 0.25 * np.arange(B); s[:, 2] = 2.0 * sym(37, 101)
    s[:, 3] = 4.0 + 6.0 * frac(29, 97); s[:, 4] = 0.1 * sym(31, 89); s[:, 5] = 0.05 * sym(41, 83); s[:, 6] = 0.2 * sym(43, 79); s[:, 7] = 0.05 * sym(47, 73)
    cmd = np.stack([np.stack([2.0 * sym(53, 71, 5 * p), 0.3 * sym(59, 67, 7 * p)], 1) for p in range(3)])
    o = outliers
    s[o[0], 3] = -2.0                                   # vx < 0
    s[o[1], 3] = 5.0; s[o[1], 4] = 1.5                  # slip tangent 0.3 > 1/8
    s[o[2], 7] = 0.7; cmd[:, o[2], 1] = 0.7             # |df| > 0.6
    s[o[3], 2] = 4.5                                    # a caller-written |psi| > 4
    s[o[4], 3:7] = (0.0, 0.0, 0.0, -1.0); cmd[:, o[4], 0] = -1.0   # standstill under braking
    s[o[5], 2] = 3.1413; s[o[5], 5] = 0.3; cmd[:, o[5], 1] = 0.1   # the heading crosses +pi within the first period
    row = np.array([1.152, 1.693, 1840.0, 3477.0, 4.0703e4, 6.4495e4, 5.0, 5.0])
    plant = row[None, :] * (1.0 + 0.2 * np.stack([sym(61 + 2 * c, 103, c) for c in range(8)], 1))
    # negative; 0; 0 < r < n; exactly n; q >= 1 with r > 0; (DEPTH - 1) n; beyond it twice
    delay = np.array([-3, 0, 4, n, n + 3, 2 * n, 2 * n + 5, 3 * n, 1000], dtype=np.int32)[np.arange(B) % 9]
    return s, cmd, plant, delay


def plant_runs():
    """(name, entry, n_updates, outliers, road or None, with road_stat)"""
    runs = []
    for n in (10, 7):
        for oname, o in (("tail", OUTLIERS_TAIL), ("wave0", OUTLIERS_WAVE0)):
            for entry in ("fixed", "plant", "queue"):
                runs.append(("%s_n%d_%s" % (entry, n, oname), entry, n, o, None, False))
            for rname in ROADS:
                runs.append(("road_%s_n%d_%s" % (rname, n, oname), "road", n, o, rname, True))
    for rname in ROADS:
        runs.append(("road_%s_nostat_n7_wave0" % rname, "road", 7, OUTLIERS_WAVE0, rname, False))
    return runs


def run_plant(entry, n, outliers, road, stat):
    """three consecutive periods from period 0 -> (digest of the inputs, digest of state (+ road_stat) after each period and of the final ring)"""
    import torch
    from mkz_mpc_path_follower_amd import _lib
    from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator
    s0, cmd, plant, delay = plant_inputs(n, outliers)
    hin = digest(digest(digest(digest(fresh(), s0), cmd.transpose(1, 0, 2)), plant), delay)
    if entry == "fixed":
        sim = VehicleSimulator(B)
    elif entry == "plant":
        sim = VehicleSimulator(B, plant=plant, cmd_delay=delay)
    else:
        rows = None if road is None else np.tile(np.array(ROADS[road]), (B, 1))
        sim = VehicleSimulator(B, plant=plant, cmd_delay=delay, cmd_queue_depth=DEPTH, road=rows)
        if road is not None:
            hin = digest(hin, rows)
    sim.state.copy_(dev(s0))
    h = fresh()
    for p in range(3):
        sim.cmd.copy_(dev(cmd[p]))
        if road is not None and not stat:   # the class always passes its road_stat: the call without one goes to the library directly
            L, vp = _lib.load(), C.c_void_p
            _lib.check(L.kmpc_sim_advance_road(0, B, vp(sim.state.data_ptr()), vp(sim.cmd.data_ptr()), vp(sim.plant.data_ptr()), vp(sim.road.data_ptr()),
                                               vp(sim.cmd_delay.data_ptr()), vp(sim.cmd_queue.data_ptr()), DEPTH, p, n, None,
                                               vp(torch.cuda.current_stream().cuda_stream)))
        else:
            sim._update_vehicle_model(n)
        torch.cuda.synchronize()
        h = digest(h, host(sim.state))
        if road is not None and stat:
            h = digest(h, host(sim.road_stat))
    if sim.cmd_held is not None:
        h = digest(h, host(sim.cmd_held))
    if sim.cmd_queue is not None:
        h = digest(h, host(sim.cmd_queue).transpose(1, 0, 2))
    return fold(hin), h


# ---------------------------------------------------------------- the measurement stage
def sense_inputs():
    i = np.arange(B)
    st = np.zeros((5, B, 8))
    for p in range(5):
        st[p, :, 0] = 10.0 + 0.5 * i + 0.6 * p; st[p, :, 1] = -20.0 + 0.25 * i - 0.3 * p; st[p, :, 2] = 2.0 * sym(37, 101) + 0.01 * p
        st[p, :, 3] = 3.0 + 5.0 * frac(29, 97) + 0.05 * p; st[p, :, 4:8] = 0.01 * (p + 1)
    st[:, i % 5 == 0, 2] = 3.1415; st[:, i % 10 == 5, 2] = -3.1415          # within the heading noise (0.02 rad) of +-pi
    st[:, i % 7 == 3, 3] = 0.05                                             # with bias_v = -0.2: a speed below 0
    sigma = np.tile(np.array([0.3, 0.2, 0.02, 0.1]), (B, 1))
    sigma[i % 4 == 0] = 0.0; sigma[i % 4 == 1, 2:4] = 0.0; sigma[i % 4 == 2, 0:2] = 0.0   # a channel pair all zero / only one pair / both
    sigma[i % 8 == 7, 1] = 0.0; sigma[i % 8 == 7, 2] = 0.0                                  # one channel of a pair zero, the other not
    bias = np.stack([0.1 * sym(53, 71), 0.1 * sym(59, 67), 0.01 * sym(61, 103), 0.05 * sym(41, 83)], 1)
    bias[i % 7 == 3, 3] = -0.2
    delay = np.array([0, 1, 5], dtype=np.int32)[i % 3]                      # 5 > depth - 1 = 2: clamped by the kernel
    return st, sigma, bias, delay


def run_sense(delayed):
    import torch
    from mkz_mpc_path_follower_amd.vehicle_sim import SensorModel
    st, sigma, bias, delay = sense_inputs()
    hin = digest(digest(digest(digest(fresh(), st.transpose(1, 0, 2)), sigma), bias), delay)
    if delayed:
        sen = SensorModel(B, sigma=sigma, bias=bias, seed=0x1234567890ABCDEF, id_base=(1 << 32) + 5, meas_delay=np.minimum(delay, 2), depth=3)
        sen.meas_delay.copy_(dev(delay))
    else:
        sen = SensorModel(B, sigma=sigma, bias=bias, seed=0x1234567890ABCDEF, id_base=(1 << 32) + 5)
    h = fresh()
    for p in range(5):
        est = sen.sense(dev(st[p]), p)
        torch.cuda.synchronize()
        h = digest(h, host(est))
    if delayed:
        h = digest(h, host(sen.truth_ring).transpose(1, 0, 2))
    return fold(hin), h


# ---------------------------------------------------------------- delay compensation
GRID = np.array([(d, lm) for d in range(36) for lm in range(3)])   # tests/test_latency.py's delay grid: 108 pairs, two batches of 70
LAT_CASES = [("grid0_n10", 0, 10), ("grid1_n10", 38, 10), ("grid0_n7", 0, 7)]
LAT_PERIODS = (0, 1, 3, 9)     # depth is 7 (n = 10) or 8 (n = 7): the first three come before the log is filled
PSI_CAP = 0.2


def latency_inputs(first):
    i = np.arange(B)
    g = GRID[first:first + B]
    z = np.stack([5.0 + 0.5 * i, -3.0 + 0.25 * i, 2.0 * sym(37, 101), 6.0 * frac(29, 97)], 1)
    z[i % 9 == 4, 2] = 3.14                                                 # the prediction wraps
    rec = np.zeros((B, 40))
    rec[:, 0:4] = z + 0.01 * np.stack([sym(53, 71), sym(59, 67), 0.1 * sym(61, 103), sym(41, 83)], 1)
    rec[:, 4] = 0.1 * sym(43, 79); rec[:, 5] = 0.04 * sym(47, 73); rec[:, 6] = 0.6 * sym(31, 89)
    rec[i % 7 == 2, 4] = 0.3; rec[i % 7 == 4, 4] = -0.35                    # dpsi beyond psi_cap, either sign
    rec[:, 35] = 3.0
    rec[i % 5 == 0, 35] = 0.0                                               # fresh records: est comes back
    return g[:, 0].astype(np.int32), g[:, 1].astype(np.int32), z, rec


def latency_hist(depth):
    return np.stack([np.stack([2.0 * sym(53, 71, 5 * p), 0.3 * sym(59, 67, 7 * p)], 1) for p in range(depth)])


def run_latency(first, n):
    import torch
    from mkz_mpc_path_follower_amd.vehicle_sim import DisturbanceObserver, LatencyCompensator
    d, lm, z, rec = latency_inputs(first)
    comp = LatencyCompensator(B, cmd_delay=d, meas_delay=lm, n_updates=n, depth=2 + -(-35 // n) + 1, disturbances=True)
    comp.max_cmd_delay, comp.max_meas_delay = 35, 2   # the grid's, whichever part of it this batch holds
    ob = DisturbanceObserver(B, psi_cap=PSI_CAP)
    hist = latency_hist(comp.depth)
    comp.cmd_hist.copy_(dev(hist))
    ob.record.copy_(dev(rec))
    hin = digest(digest(digest(digest(digest(fresh(), d), lm), z), rec), hist.transpose(1, 0, 2))
    zd = dev(z)
    hu, hp, hd = fresh(), fresh(), fresh()
    for p in LAT_PERIODS:
        u, zp, zq = comp.filter_input(p), comp.predict(zd, p), comp.predict_disturbed(ob, zd, p)
        torch.cuda.synchronize()
        hu, hp, hd = digest(hu, host(u)), digest(hp, host(zp)), digest(hd, host(zq))
    return fold(hin), hu, hp, hd


# ---------------------------------------------------------------- estimator, observer, command offset
def filter_inputs():
    """four calls: z [4,B,4], u [4,B,2].  Lanes by i % 6: 1 -- x far off in call 2 (gated); 2 -- y NaN in call 1 (dropout); 3 -- x inf in call 0
    (the record stays fresh); 4 -- an infinite acceleration in call 2 (the record resets); 5 -- 0.5 m/s, below the observer's v_min"""
    i = np.arange(B)
    z, u = np.zeros((4, B, 4)), np.zeros((4, B, 2))
    v = 3.0 + 5.0 * frac(29, 97)
    v[i % 6 == 5] = 0.5
    for k in range(4):
        z[k, :, 0] = 5.0 + 0.5 * i + 0.1 * k * v + 0.05 * sym(53, 71, k); z[k, :, 1] = -3.0 + 0.25 * i + 0.02 * k + 0.05 * sym(59, 67, k)
        z[k, :, 2] = 0.4 * sym(37, 101) + 0.005 * k + 0.01 * sym(61, 103, k); z[k, :, 3] = v + 0.02 * k + 0.05 * sym(41, 83, k)
        u[k, :, 0] = 0.4 * sym(43, 79, k); u[k, :, 1] = 0.1 * sym(47, 73, k)
    z[:, i % 12 == 0, 2] += 3.13                                            # headings at the wrap
    z[2, i % 6 == 1, 0] += 50.0
    z[1, i % 6 == 2, 1] = np.nan
    z[0, i % 6 == 3, 0] = np.inf
    u[2, i % 6 == 4, 0] = np.inf
    latch = (i % 4 == 0).astype(np.uint8)
    cmd = np.stack([np.stack([2.0 * sym(53, 71, 5 * k), 0.3 * sym(59, 67, 7 * k)], 1) for k in range(4)])
    return z, u, latch, cmd


def run_filters():
    import torch
    from mkz_mpc_path_follower_amd.vehicle_sim import DisturbanceObserver, Estimator
    z, u, latch, cmd = filter_inputs()
    hin = digest(digest(digest(digest(fresh(), z.transpose(1, 0, 2)), u.transpose(1, 0, 2)), latch), cmd.transpose(1, 0, 2))
    est = Estimator(B, gate=3.0)
    ob = DisturbanceObserver(B, gate=3.0, acc_cap=0.01, df_cap=0.0005, psi_cap=0.002)   # small caps: some lanes clip, some do not
    lt = dev(latch)
    he, ho, hc = fresh(), fresh(), fresh()
    for k in range(4):
        zk, uk, ck = dev(z[k]), dev(u[k]), dev(cmd[k])
        e = est.update(zk, uk)
        o = ob.update(zk, uk)
        ob.offset(ck, lt)
        torch.cuda.synchronize()
        for a in (e, est.record, est.innov, est.flags):
            he = digest(he, host(a))
        for a in (o, ob.record, ob.dist, ob.innov, ob.flags):
            ho = digest(ho, host(a))
        hc = digest(hc, host(ck))
    return fold(hin), he, ho, hc


# ---------------------------------------------------------------- both closed loops, every stage on
LOOP_NV, LOOP_STEPS, LOOP_VT = 8, 5, 6.0
LOOP_KEYS = ("state", "cmd", "status", "latch", "est", "est_filt", "dist", "est_pred")


def run_loop(kind, X0, Y0, Psi0):
    """8 vehicles, N = 8, 5 periods on path1: a sensor with noise and a fix one period old, the observer, LatencyCompensator(disturbances=True)
    fed from its log, a command queue of depth 2 with 7 updates of delay, and a road slippery enough to saturate -> run(history=True)'s arrays"""
    import torch
    import scenario as S
    from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop, ClosedLoopFrenet
    from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory
    from mkz_mpc_path_follower_amd.vehicle_sim import DisturbanceObserver, LatencyCompensator, SensorModel, VehicleSimulator, road_params
    nv = LOOP_NV
    arr, lat0, lon0 = S.path_arrays("path1_decimated.npz")
    grt = GPSRefTrajectory(arrays=arr, traj_horizon=8, traj_dt=0.2, lat0=lat0, lon0=lon0)
    sim = VehicleSimulator(nv, X0=X0, Y0=Y0, Psi0=Psi0, cmd_delay=7, cmd_queue_depth=2,
                           road=road_params(nv, mu=0.05, a_lat=1.5, a_long=-0.3, df_offset=0.02, acc_gain=0.9))
    sim.state[:, 3] = LOOP_VT
    kw = dict(sensor=SensorModel(nv, sigma=(0.3, 0.3, 0.02, 0.1), seed=7, meas_delay=1), observer=DisturbanceObserver(nv),
              compensator=LatencyCompensator(nv, cmd_delay=7, meas_delay=1, disturbances=True), estimator_input="history")
    loop = ClosedLoopFrenet(grt, sim, 8, LOOP_VT, **kw) if kind == "frenet" else ClosedLoop(grt, sim, N=8, target_vel=LOOP_VT, **kw)
    h = loop.run(LOOP_STEPS, history=True)
    torch.cuda.synchronize()
    out = {k: host(h[k]) for k in LOOP_KEYS}
    out["sat"] = host(sim.road_stat)
    return out


# ================================================================ tests/golden/plant_family_parent.npz
# The second file (tests/test_plant_family_parent.py): the pedal-driven plant and the measurement stage with faults, recorded on the build before the
# plant kernels were given one body and the measurement kernels one truth-ring fetch.  Same conventions as above.

# ---------------------------------------------------------------- the pedal-driven plant
DRIVE_ROADS = ("neutral", "both")
DRIVE_ROW = np.array([6000.0, 120e3, 5.0, 5.0, 0.15, 4e-4, 14.8, 0.33])            # kmpc_drive_default
LLC_ROW = np.array([0.8, 0.4, 1.0, 1.0, 14.8, 1847.78, 0.1, 0.33])                 # kmpc_llc_default


def drive_runs():
    """(name, n_updates, outliers, road, with road_stat)"""
    return [("drive_%s_%s_n%d_%s" % (rname, "stat" if stat else "nostat", n, oname), n, o, rname, stat)
            for n in (10, 7) for oname, o in (("tail", OUTLIERS_TAIL), ("wave0", OUTLIERS_WAVE0)) for rname in DRIVE_ROADS for stat in (True, False)]


def drive_inputs():
    """non-default powertrain and controller rows, spread per lane, and the speeds the controllers' records start from (V_LAST)"""
    drive = DRIVE_ROW[None, :] * (1.0 + 0.2 * np.stack([sym(61 + 2 * c, 107, c + 3) for c in range(8)], 1))
    llc = LLC_ROW[None, :] * (1.0 + 0.2 * np.stack([sym(67 + 2 * c, 109, c + 5) for c in range(8)], 1))
    v_last = 4.0 + 6.0 * frac(29, 97) - 0.25
    return drive, llc, v_last


def run_drive(n, outliers, road, stat):
    """three consecutive periods from period 0 (with n = 7 the 50 Hz tick's parity flips between periods) -> (digest of the inputs, digest of
    state, llc_rec (+ road_stat) after each period and of the final ring)"""
    import torch
    from mkz_mpc_path_follower_amd import _lib
    from mkz_mpc_path_follower_amd.vehicle_sim import LowLevelController, VehicleSimulator, check_drive_rows, check_llc_rows
    s0, cmd, plant, delay = plant_inputs(n, outliers)
    drive, llc_rows, v_last = drive_inputs()
    rows = np.tile(np.array(ROADS[road]), (B, 1))
    hin = fresh()
    for a in (s0, cmd.transpose(1, 0, 2), plant, delay, rows, drive, llc_rows, v_last):
        hin = digest(hin, a)
    llc = LowLevelController(B, v0=v_last)          # a record that is not fresh: V_LAST set
    llc.params.copy_(dev(check_llc_rows(llc_rows)))
    sim = VehicleSimulator(B, plant=plant, cmd_delay=delay, cmd_queue_depth=DEPTH, road=rows, drive=check_drive_rows(drive), llc=llc)
    sim.state.copy_(dev(s0))
    h = fresh()
    for p in range(3):
        sim.cmd.copy_(dev(cmd[p]))
        if not stat:   # the class always passes its road_stat: the call without one goes to the library directly
            L, vp = _lib.load(), C.c_void_p
            _lib.check(L.kmpc_sim_advance_drive(0, B, vp(sim.state.data_ptr()), vp(sim.cmd.data_ptr()), vp(sim.plant.data_ptr()), vp(sim.road.data_ptr()),
                                                vp(sim.drive.data_ptr()), vp(llc.params.data_ptr()), vp(llc.rec.data_ptr()),
                                                vp(sim.cmd_delay.data_ptr()), vp(sim.cmd_queue.data_ptr()), DEPTH, p, n, None,
                                                vp(torch.cuda.current_stream().cuda_stream)))
        else:
            sim._update_vehicle_model(n)
        torch.cuda.synchronize()
        h = digest(digest(h, host(sim.state)), host(llc.rec))
        if stat:
            h = digest(h, host(sim.road_stat))
    h = digest(h, host(sim.cmd_queue).transpose(1, 0, 2))
    return fold(hin), h


# ---------------------------------------------------------------- the measurement stage with faults
FAULT_PERIODS, FAULT_DEPTH, FAULT_SEED, FAULT_ID_BASE = 4, 3, 0x1234567890ABCDEF, (1 << 32) + 5
FAULT_NEUTRAL = np.array([0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, np.inf, 0], dtype=np.float64)   # kmpc_sense_faults_default
F_OUTLIER, F_BLIND, F_FRESH, F_RESET = 8, 16, 32, 64                                                 # KMPC_FAULT_FLAG_*; source s silent: 1 << s


def fault_inputs():
    """-> (states [5,B,8], sensor [B,8], faults [B,16], rec0 [B,16], meas_delay [B]).  The fault row of lane i belongs to group g = i % 7, its
    source (0 GPS, 1 IMU, 2 speed) is s = (i // 7) % 3; every record but groups 2 and 6 starts fresh, so period 0 delivers every source:
      0 neutral
      1 source s: P_LOSE = P_REGAIN = 1 -- lost in period 1, regained in 2, lost in 3, whatever the draw
      2 all three sources on a chain by the draw (P_LOSE = P_REGAIN = 0.5), from a record in use: 5 calls counted, chain word i % 8
      3 a window on source s: periods 1 and 2
      4 outliers: P_OUTLIER 1 (s = 0) or 0.5, OUTLIER_SIGMA 3 m
      5 a window on source s over periods 1 ... 3 with MAX_AGE 1: blind from period 2
      6 a record that resets: COUNT -1 (s = 0), COUNT NaN (1), CHAIN 8 (2), the other words in use; then GPS lost in period 1"""
    st, sigma, bias, _ = sense_inputs()
    i = np.arange(B)
    g, s = i % 7, (i // 7) % 3
    f = np.tile(FAULT_NEUTRAL, (B, 1))
    rec = np.zeros((B, 16))
    for b in range(B):
        if g[b] == 1:
            f[b, 0 + s[b]] = 1.0
        elif g[b] == 2:
            f[b, 0:6] = 0.5
        elif g[b] == 3:
            f[b, 6 + s[b]], f[b, 9 + s[b]] = 1.0, 2.0
        elif g[b] == 4:
            f[b, 12], f[b, 13] = (1.0 if s[b] == 0 else 0.5), 3.0
        elif g[b] == 5:
            f[b, 6 + s[b]], f[b, 9 + s[b]], f[b, 14] = 1.0, 3.0, 1.0
        elif g[b] == 6:
            f[b, 0] = 1.0
    used = (g == 2) | (g == 6)
    rec[used, 0:4] = st[0][used, 0:4] + 0.5
    rec[used, 4] = 5.0
    rec[used, 5] = (i % 8)[used]
    rec[used, 6:9] = ((i[:, None] % 8 >> np.arange(3)[None, :]) & 1)[used] * 2.0      # a silent source's age
    rec[used, 9:12] = 2.0; rec[used, 12:15] = 2.0; rec[used, 15] = 1.0
    rec[(g == 6) & (s == 0), 4] = -1.0
    rec[(g == 6) & (s == 1), 4] = np.nan
    rec[(g == 6) & (s == 2), 5] = 8.0
    delay = np.array([-1, 0, 1, FAULT_DEPTH - 1, FAULT_DEPTH + 3], dtype=np.int32)[i % 5]
    return st, np.concatenate([sigma, bias], 1), f, rec, delay


def fault_events(flags):
    """flags [FAULT_PERIODS,B] int32 of a run over fault_inputs() -> dict event -> bool: what the rows are there to produce"""
    i = np.arange(B)
    g, s = i % 7, (i // 7) % 3
    bit = (flags[:, :] >> s[None, :]) & 1           # the lane's own source silent
    ev = {}
    for k, name in enumerate(("gps", "imu", "spd")):
        m = (g == 1) & (s == k)
        ev["lost_and_regained_" + name] = bool(m.any() and (bit[0, m] == 0).all() and (bit[1, m] == 1).all() and (bit[2, m] == 0).all())
    m = g == 3
    ev["window"] = bool((bit[0, m] == 0).all() and (bit[1, m] == 1).all() and (bit[2, m] == 1).all() and (bit[3, m] == 0).all())
    ev["outlier"] = bool((flags[:, g == 4] & F_OUTLIER).any())
    ev["blind"] = bool((flags[2:, g == 5] & F_BLIND).all() and not (flags[:2] & F_BLIND).any())
    ev["reset"] = bool((flags[0, g == 6] & F_RESET).all() and not (flags[:, g != 6] & F_RESET).any() and not (flags[1:] & F_RESET).any())
    ev["chain_by_the_draw"] = bool((flags[:, g == 2] & 7).any() and ((flags[:, g == 2] & 7) != 7).any())
    return ev


def run_faults(ring):
    """FAULT_PERIODS periods from period 0 -> (digest of the inputs, digest of z, held, flags, blind, fault_rec after each period and of the final
    ring, the flags [FAULT_PERIODS,B] in full)"""
    import torch
    from mkz_mpc_path_follower_amd.vehicle_sim import SensorModel
    st, sensor, faults, rec0, delay = fault_inputs()
    hin = fresh()
    for a in (st.transpose(1, 0, 2), sensor, faults, rec0, delay):
        hin = digest(hin, a)
    kw = dict(meas_delay=np.clip(delay, 0, FAULT_DEPTH - 1), depth=FAULT_DEPTH) if ring else {}
    sen = SensorModel(B, sigma=sensor[:, 0:4], bias=sensor[:, 4:8], seed=FAULT_SEED, id_base=FAULT_ID_BASE, faults=faults, **kw)
    if ring:
        sen.meas_delay.copy_(dev(delay))       # the raw delays: the kernel clamps
    sen.fault_record.copy_(dev(rec0))
    h, flags = fresh(), []
    for p in range(FAULT_PERIODS):
        held = sen.sense(dev(st[p]), p)
        torch.cuda.synchronize()
        for a in (sen.z, held, sen.flags, sen.blind, sen.fault_record):
            h = digest(h, host(a))
        flags.append(host(sen.flags).copy())
    if ring:
        h = digest(h, host(sen.truth_ring).transpose(1, 0, 2))
    return fold(hin), h, np.array(flags, dtype=np.int32)


def fault_flags_cpu(ring):
    """the same run on tests/sensor_fault_ref.py (numpy, no GPU) -> flags [FAULT_PERIODS,B] int32"""
    import sensor_fault_ref as SF
    st, sensor, faults, rec, delay = fault_inputs()
    flags = []
    for p in range(FAULT_PERIODS):
        o = (SF.sense_faults_delayed(st, sensor, faults, rec, FAULT_SEED, p, delay, FAULT_DEPTH, FAULT_ID_BASE) if ring else
             SF.sense_faults(st[p], sensor, faults, rec, FAULT_SEED, p, FAULT_ID_BASE))
        rec = o["rec"]
        flags.append(o["flags"])
    return np.array(flags, dtype=np.int32)
