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
