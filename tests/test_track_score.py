"""Tracking errors per vehicle on the device and the running score record (kmpc_track_score_batch / _fleet, ref_traj.track_score_batch,
ClosedLoop.run / ClosedLoopFrenet.run, score_summary) against the numpy restatement tests/track_score_ref.py.

CPU: the restatement against scenario.cross_track, against the reference's own nearest-sample formulation (scipy cdist + argmin) and against
scenario.summarize; the new symbols; the argument checks without a GPU.
GPU: the kernels against numpy on the five-path set of fleet_scenario plus a path with repeated samples (M = 2235, 2, 2198, 65, 2209, 63); the accumulation over
five calls; run() against step() bit for bit and its score against the restatement on the downloaded history, Cartesian fleet, Frenet loop and a
weight sweep in one loop.

BOUNDS on e_ct, e_near, s_along and the record's maxima against numpy.  Coordinates are <= 312 m, so a difference of two of them carries <= 2^-45 =
2.8e-14 m of rounding per operand and the distance a few 1e-13 m at worst; FMA contraction in the segment part moves the last bits.  Each bound is 10 x the
largest difference its tests measured on the MI355X (they print it before they assert), never above 1e-9 m (the projection bound of DESIGN.md section 6):
  BOUND_KERNEL  test_kernel_matches_numpy: e_ct 8.882e-16, e_near 0, s_along 1.776e-15, distance to the reported segment - minimum 0      -> 1.8e-14 m
  BOUND_ACC     test_accumulation_over_five_calls: maxima against the accumulation of numpy's errors 8.882e-16                              -> 8.9e-15 m
  BOUND_LOOP    the two run-against-steps tests: maxima 2.220e-16, s_along of the last state 0 (arclengths up to 523 m)                     -> 2.3e-15 m
Every test that uses a bound has been measured; none is left at 1e-9.  e_psi is three additions: 1e-12 rad (measured 0).
The mixed-fleet and Frenet histories keep 1.1e-2 m and 6.2e-5 m between any |e_ct| and the settle tolerance 0.5 m (precondition > 1e-6 m, asserted), so 0.5 stays.
Sums of squares against numpy's errors are compared at 1e-12 relative PLUS 2 * bound * sum |e| (a few 1e-14 at these bounds): the restatement's errors
themselves may differ from the kernel's by the bound per state, and (e + delta)^2 - e^2 = 2 e delta + delta^2."""
import ctypes as C

import numpy as np
import pytest

import fleet_scenario as F
import scenario as S
import track_score_ref as R

BOUND_KERNEL = 1.8e-14   # m, 10 x 1.776e-15
BOUND_ACC = 8.9e-15      # m, 10 x 8.882e-16
BOUND_LOOP = 2.3e-15     # m, 10 x 2.220e-16
BOUND_PSI = 1e-12   # rad
H = 8


def six_paths():
    """fleet_scenario.five_paths() plus path1's samples 200 ... 260 with samples 10 and 30 each repeated once: two zero-length segments (the fixtures have
    none: their shortest segment is 7.5e-5 m)"""
    d = F.path_dict(0, 200, 261)
    keep = np.sort(np.concatenate([np.arange(61), [10, 30]]))
    sixth = {k: (np.asarray(v)[keep] if k in ("t", "lat", "lon", "psi") else v) for k, v in d.items()}
    return F.five_paths() + [sixth]


def trajectories(paths):
    from mkz_mpc_path_follower_amd.ref_traj import path_arrays
    return [np.column_stack(path_arrays(p["t"], p["lat"], p["lon"], p["psi"], p["lat0"], p["lon0"])) for p in paths]


def poses_for(tr, rng):
    """about a dozen poses on one path [M,7] -> [n,3]"""
    M = len(tr)
    X, Y, psi = tr[:, 4], tr[:, 5], tr[:, 3]

    def frame(j):   # unit tangent and left normal of segment j (the next one of non-zero length)
        while True:
            d = np.array([X[j + 1] - X[j], Y[j + 1] - Y[j]])
            if np.hypot(*d) > 0 or j + 2 >= M:
                break
            j += 1
        t = d / max(np.hypot(*d), 1e-300)
        return t, np.array([-t[1], t[0]])
    out = []
    i = M // 2
    out.append((X[i], Y[i], psi[i]))                                               # on a vertex
    j = min(M // 3, M - 2)
    t, n = frame(j)
    mid = np.array([0.5 * (X[j] + X[j + 1]), 0.5 * (Y[j] + Y[j + 1])])
    for side in (+0.3, -0.3):                                                       # mid-segment, 0.3 m to the left and to the right: the sign
        out.append((*(mid + side * n), psi[j] + 0.02))
    t, n = frame(0)
    out.append((*(np.array([X[0], Y[0]]) - 5.0 * t + 0.3 * n), psi[0]))             # 5 m before the first sample: the clamp at s = 0 (0.3 m aside: a defined sign)
    t, n = frame(M - 2)
    out.append((*(np.array([X[-1], Y[-1]]) + 5.0 * t - 0.3 * n), psi[-1]))          # 5 m beyond the last: the clamp at s = 1
    for k, off in ((10, (0.2, -0.1)), (11, (-0.05, 0.15)), (30, (-0.2, 0.1)), (31, (0.0, 0.0))):   # next to (and on) the repeated samples of the sixth path
        k = min(k, M - 1)
        out.append((X[k] + off[0], Y[k] + off[1], psi[k] - 0.03))
    k = min(64, M - 1)
    t, n = frame(min(k, M - 2))
    out.append((*(np.array([X[k], Y[k]]) + 0.1 * t + 0.1 * n), psi[k]))             # nearest sample 64, the last, on the M = 65 path: the second trip of lane 0
    k = int(np.argmin(psi))
    out.append((X[k] + 0.05, Y[k], np.pi - 0.01))                                   # heading pi - 0.01 against the path's most negative heading: fix_heading
    k = int(np.argmax(psi))
    out.append((X[k], Y[k] + 0.05, -np.pi + 0.01))
    for k in rng.integers(0, M, 3):
        out.append((X[k] + rng.normal(0, 1.5), Y[k] + rng.normal(0, 1.5), psi[k] + rng.normal(0, 0.3)))
    return np.array(out, dtype=np.float64)


def build_poses(trs, seed=5):
    rng = np.random.default_rng(seed)
    pose, pid = [], []
    for p, tr in enumerate(trs):
        q = poses_for(tr, rng)
        pose.append(q); pid += [p] * len(q)
    return np.concatenate(pose), np.array(pid, dtype=np.int32)


def numpy_errors(trs, pose, pid):
    """restatement per vehicle -> dict of arrays [B]; vehicles with a bad id or a non-finite pose: zeros and seg = closest = -1"""
    B = len(pid)
    out = dict(e_ct=np.zeros(B), e_near=np.zeros(B), e_psi=np.zeros(B), s_along=np.zeros(B), seg=-np.ones(B, dtype=np.int64), closest=-np.ones(B, dtype=np.int64),
               ok=np.zeros(B, dtype=bool))
    for p, tr in enumerate(trs):
        sel = np.where((pid == p) & np.isfinite(pose).all(1))[0]
        if len(sel):
            e = R.errors(tr, pose[sel, 0], pose[sel, 1], pose[sel, 2])
            for k in ("e_ct", "e_near", "e_psi", "s_along", "seg", "closest"):
                out[k][sel] = e[k]
            out["ok"][sel] = True
    return out


# ---------------------------------------------------------------- CPU
def test_restatement_equals_cross_track_and_the_references_nearest_sample():
    """unsigned polyline distance = scenario.cross_track's; nearest-sample distance and index = scipy cdist + argmin (plot_path_tracking_error.py:30-32) on
    200 seeded points around each fixture path; the signs of the two sides of a segment"""
    import scipy.spatial.distance as ssd
    rng = np.random.default_rng(3)
    for p in range(3):
        tr = F.trajectory(p)
        idx = rng.integers(0, len(tr), 200)
        x, y = tr[idx, 4] + rng.normal(0, 2.0, 200), tr[idx, 5] + rng.normal(0, 2.0, 200)
        e = R.errors(tr, x, y, tr[idx, 3] + rng.normal(0, 0.3, 200))
        ect, seg = S.cross_track(tr[:, 4:6], x, y)
        assert np.array_equal(np.abs(e["e_ct"]), ect) and np.array_equal(e["seg"], seg)
        dist = ssd.cdist(tr[:, 4:6], np.stack([x, y], 1))
        ci = np.argmin(dist, axis=0)
        assert np.array_equal(ci, e["closest"])
        assert np.abs(dist[ci, np.arange(200)] - e["e_near"]).max() <= 1e-12
        assert (e["e_near"] >= np.abs(e["e_ct"]) - 1e-12).all()                     # a sample is a point of the polyline
        assert (np.abs(e["e_psi"]) <= np.pi + 1e-12).all()
        assert (e["s_along"] >= 0).all() and (e["s_along"] <= tr[-1, 6]).all()
    tr = F.trajectory(0)
    j = 700
    d = tr[j + 1, 4:6] - tr[j, 4:6]
    n = np.array([-d[1], d[0]]) / np.hypot(*d)
    mid = 0.5 * (tr[j, 4:6] + tr[j + 1, 4:6])
    e = R.errors(tr, [mid[0] + 0.3 * n[0], mid[0] - 0.3 * n[0]], [mid[1] + 0.3 * n[1], mid[1] - 0.3 * n[1]], [0.0, 0.0])
    assert abs(e["e_ct"][0] - 0.3) < 1e-3 and abs(e["e_ct"][1] + 0.3) < 1e-3      # left of travel positive (the path bends: not exactly 0.3)
    p = np.array([2 * np.pi - 0.01, -4.0, 0.5, np.pi])
    assert np.array_equal(R.fix_heading(p), [p[0] - 2 * np.pi, p[1] + 2 * np.pi, p[2], p[3]])    # pi and -pi tie: the first candidate stays


def test_accumulation_agrees_with_summarize():
    """the plain-Python record over a synthetic history against scenario.summarize on the fields that has"""
    tr = F.trajectory(0)
    rng = np.random.default_rng(4)
    T = 50
    k = 300 + 3 * np.arange(T + 1)
    off = 1.2 * np.exp(-np.arange(T + 1) / 8.0) + 0.01 * rng.normal(size=T + 1)    # decays through 0.5 m
    state = np.stack([tr[k, 4] + off, tr[k, 5] - 0.5 * off, tr[k, 3] + 0.1 * off], 1)
    cmd = np.stack([rng.uniform(-1, 1, T), rng.uniform(-0.3, 0.3, T)], 1)
    latch = np.arange(T) >= 41
    cmd[latch] = (-1.0, 0.0)
    status = np.zeros(T, dtype=np.int64); status[7] = 1
    iters = rng.integers(3, 9, T)
    rec, e = R.accumulate_history(tr, state, cmd, status, iters, latch, 0.5)
    sm = S.summarize(tr, state, cmd, latch)
    assert np.abs(np.abs(e["e_ct"]) - 0.5).min() > 1e-6
    assert rec["settle_index"] == round(sm["t_converged"] / 0.1) and rec["settle_index"] > 0
    assert rec["max_dacc"] == sm["max_dacc"] and rec["max_ddf"] == sm["max_ddf"]
    assert rec["n_live"] == sm["n_live"] == 41 and rec["latch_index"] == round(sm["t_stop"] / 0.1) == 41
    assert rec["n"] == T + 1 and rec["n_nonopt"] == 1 and rec["sum_iters"] == iters[:41].sum() and rec["n_refused"] == 0
    assert rec["max_ect"] == sm["ect"].max() and abs(rec["sum_ect2"] - (sm["ect"] ** 2).sum()) <= 1e-12 * rec["sum_ect2"]


def test_new_symbols_are_exported_and_listed():
    from mkz_mpc_path_follower_amd import _lib, ref_traj
    L = _lib.load()
    for n in ("kmpc_track_score_init", "kmpc_track_score_batch", "kmpc_track_score_fleet"):
        assert n in _lib.EXPORTS and hasattr(L, n), n
    assert ref_traj.SCORE_FIELDS == R.FIELDS and ref_traj.SCORE_WORDS == 16
    rec = np.full((3, 16), 7.0)
    assert L.kmpc_track_score_init(rec.ctypes.data_as(C.POINTER(C.c_double)), 3) == 0
    want = np.zeros((3, 16)); want[:, 15] = -1.0
    assert np.array_equal(rec, want)
    assert L.kmpc_track_score_init(None, 3) == -1 and L.kmpc_track_score_init(None, 0) == 0 and L.kmpc_track_score_init(rec.ctypes.data_as(C.POINTER(C.c_double)), -1) == -1


def test_bad_arguments_are_refused_before_any_device_call():
    """every case answers KMPC_ERR_ARG without a GPU: the checks come before the handle is used, so a handle that is no handle (64 zero bytes) is never read"""
    from mkz_mpc_path_follower_amd import _lib
    L = _lib.load()
    fake = C.cast(C.create_string_buffer(64), C.c_void_p)
    buf = C.cast(C.create_string_buffer(256), C.c_void_p)   # never read either
    good = dict(h=fake, B=2, state=buf, stride=8, pid=buf, tol=0.5, status=None, iters=None, cmd=None, latch=None)
    cases = [dict(h=None), dict(B=-1), dict(state=None), dict(stride=2), dict(tol=float("nan")), dict(tol=float("inf")), dict(tol=-0.1),
             dict(status=buf), dict(cmd=buf, latch=buf), dict(status=buf, iters=buf, cmd=buf)]
    for c in cases:
        a = dict(good, **c)
        tail = (a["tol"], a["status"], a["iters"], a["cmd"], a["latch"], None, None, None, None, None)
        assert L.kmpc_track_score_batch(a["h"], a["B"], a["state"], a["stride"], *tail) == -1, c
        assert L.kmpc_last_error(None)
        assert L.kmpc_track_score_fleet(a["h"], a["B"], a["state"], a["stride"], a["pid"], *tail) == -1, c
    tail = (0.5, None, None, None, None, None, None, None, None, None)
    assert L.kmpc_track_score_fleet(fake, 2, buf, 8, None, *tail) == -1                       # a fleet without path ids
    assert b"null" in L.kmpc_last_error(None)
    assert L.kmpc_track_score_batch(fake, 0, None, 8, *tail) == 0 and L.kmpc_track_score_fleet(fake, 0, None, 8, None, *tail) == 0   # B = 0: no launch


# ---------------------------------------------------------------- GPU, kernel against numpy
@pytest.fixture(scope="module")
def six():
    """the six-path set, its poses with three refused vehicles in the middle, and the fleet kernel's answer (computed once) -> dict"""
    import torch
    from mkz_mpc_path_follower_amd.ref_traj import FleetRefTrajectory, fresh_score
    paths = six_paths()
    trs = trajectories(paths)
    assert [len(t) for t in trs] == [2235, 2, 2198, 65, 2209, 63]
    assert max(np.abs(t[:, 4:6]).max() for t in trs) <= 312.0
    assert (np.hypot(np.diff(trs[5][:, 4]), np.diff(trs[5][:, 5])) == 0).sum() == 2
    pose, pid = build_poses(trs)
    bad = np.array([[pose[20, 0], pose[20, 1], 0.1], [pose[40, 0], pose[40, 1], 0.2], [np.nan, pose[60, 1], 0.3]])
    at = 33
    pose_all = np.concatenate([pose[:at], bad, pose[at:]])
    pid_all = np.concatenate([pid[:at], np.array([-1, len(paths), 2], dtype=np.int32), pid[at:]]).astype(np.int32)
    refused = np.arange(at, at + 3)
    fleet = FleetRefTrajectory(paths, pid_all, traj_horizon=H)
    for a, b in zip(fleet.trajectories, trs):
        assert np.array_equal(a, b)
    B = len(pid_all)
    state = torch.full((B, 8), 123.0, dtype=torch.float64, device=fleet.device)   # the plant's layout: X, Y, psi first, row stride 8
    state[:, 0:3] = torch.as_tensor(pose_all, device=fleet.device)
    score = fresh_score(B, fleet.device)
    o = fleet.track_score_batch(state, score=score)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    return dict(paths=paths, trs=trs, fleet=fleet, pose=pose_all, pid=pid_all, refused=refused, state=state, got=got, score=score.cpu().numpy(),
                want=numpy_errors(trs, pose_all, np.where((pid_all >= 0) & (pid_all < len(paths)), pid_all, -1)))


@pytest.mark.gpu
def test_kernel_matches_numpy(six):
    import torch
    d, g, w = six, six["got"], six["want"]
    ok = w["ok"]
    assert ok.sum() == len(ok) - 3 and not ok[d["refused"]].any()
    # closest: numpy's argmin and the waypoint kernel's closest_out, exactly
    assert np.array_equal(g["closest"][ok], w["closest"][ok])
    _r, _s, c = d["fleet"].get_waypoints_batch(torch.as_tensor(np.nan_to_num(d["pose"]), device=d["fleet"].device), np.full(len(ok), 5.0), want_closest=True)
    assert np.array_equal(c.cpu().numpy()[ok], g["closest"][ok])
    assert (g["closest"][(d["pid"] == 3) & ok] >= 64).any()                            # the second trip of the M = 65 path
    err = g["err"]
    diff = {k: np.abs(err[ok, i] - w[k][ok]).max() for i, k in enumerate(("e_ct", "e_near", "e_psi", "s_along"))}
    print("largest difference to numpy: e_ct %.3e m, e_near %.3e m, e_psi %.3e rad, s_along %.3e m" % (diff["e_ct"], diff["e_near"], diff["e_psi"], diff["s_along"]))
    assert diff["e_ct"] <= BOUND_KERNEL and diff["e_near"] <= BOUND_KERNEL and diff["s_along"] <= BOUND_KERNEL
    assert diff["e_psi"] <= BOUND_PSI
    assert (np.sign(err[ok, 0]) == np.sign(w["e_ct"][ok])).all() and (err[ok, 0] > 0.25).sum() >= 6 and (err[ok, 0] < -0.25).sum() >= 6
    raw = np.array([d["trs"][p][c, 3] for p, c in zip(d["pid"][ok], w["closest"][ok])]) - d["pose"][ok, 2]   # psi_path[closest] - psi before fix_heading
    assert (np.abs(w["e_psi"][ok]) <= np.pi).all() and (raw > np.pi).sum() >= 3 and (raw < -np.pi).sum() >= 3   # both +-2 pi candidates win somewhere
    # seg: a vertex makes two segments tie, so no index comparison -- the distance to the reported segment is the minimum
    worst = 0.0
    for p, tr in enumerate(d["trs"]):
        sel = np.where((d["pid"] == p) & ok)[0]
        seg = g["seg"][sel]
        assert (seg >= 0).all() and (seg <= len(tr) - 2).all()
        e, _s, _c = R.segment_point(tr[:, 4:6], seg, d["pose"][sel, 0], d["pose"][sel, 1])
        worst = max(worst, np.abs(e - np.abs(w["e_ct"][sel])).max())
    print("distance to the reported segment - minimum: %.3e m" % worst)
    assert worst <= BOUND_KERNEL
    assert np.isfinite(err).all() and np.isfinite(d["score"]).all()
    # the record after one geometry-only call
    sc = d["score"]
    assert (sc[ok, 0] == 1).all() and (sc[ok, 7] == 0).all() and (sc[:, 8:15] == 0).all() and (sc[:, 15] == -1).all()
    assert np.array_equal(sc[ok, 2], np.abs(err[ok, 0])) and np.array_equal(sc[ok, 5], err[ok, 1]) and np.array_equal(sc[ok, 4], np.abs(err[ok, 2]))


@pytest.mark.gpu
def test_refused_vehicles_are_contained(six):
    """path_id -1, path_id P and a NaN x: zero row, seg = closest = -1, only the refused count moves; every neighbour's outputs are those of a launch
    without them"""
    import torch
    from mkz_mpc_path_follower_amd.ref_traj import FleetRefTrajectory, fresh_score
    d, g = six, six["got"]
    r = d["refused"]
    assert (g["err"][r] == 0).all() and (g["seg"][r] == -1).all() and (g["closest"][r] == -1).all()
    want = np.zeros((3, 16)); want[:, 7] = 1; want[:, 15] = -1
    assert np.array_equal(d["score"][r], want)
    keep = np.setdiff1d(np.arange(len(d["pid"])), r)
    fleet = FleetRefTrajectory(d["paths"], d["pid"][keep], traj_horizon=H)
    score = fresh_score(len(keep), fleet.device)
    o = fleet.track_score_batch(d["state"][torch.as_tensor(keep, device=fleet.device)].contiguous(), score=score)
    for k in ("err", "seg", "closest"):
        assert np.array_equal(o[k].cpu().numpy(), g[k][keep]), k
    assert np.array_equal(score.cpu().numpy(), d["score"][keep])
    fleet.close()


@pytest.mark.gpu
def test_single_path_kernel_equals_the_fleet_kernel(six):
    """per path, bit for bit; the single-path call reads a pose [n,3] (row stride 3), the fleet call the plant's state [B,8]"""
    import torch
    from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory, fresh_score
    d, g = six, six["got"]
    seen = 0
    for p, src in enumerate(d["paths"]):
        sel = np.where((d["pid"] == p) & np.isfinite(d["pose"]).all(1))[0]
        grt = GPSRefTrajectory(arrays=src, traj_horizon=H, lat0=src["lat0"], lon0=src["lon0"])
        score = fresh_score(len(sel), grt.device)
        o = grt.track_score_batch(torch.as_tensor(d["pose"][sel], device=grt.device), score=score)
        for k in ("err", "seg", "closest"):
            assert np.array_equal(o[k].cpu().numpy(), g[k][sel]), (p, k)
        assert np.array_equal(score.cpu().numpy(), d["score"][sel]), p
        seen += len(sel)
        grt.close()
    assert seen == len(d["pid"]) - 3


@pytest.mark.gpu
def test_accumulation_over_five_calls(six):
    """call 0 geometry only, calls 1 ... 4 with a command side: vehicle 5's latch comes up at call 3, vehicle 7 is not Optimal at call 2, vehicle 9 has a NaN y
    at call 2 only.  The record against the plain-Python accumulation: of numpy's errors (counts exact, maxima within BOUND_ACC, sums within 1e-12 relative
    + 2 BOUND_ACC sum |e|) and of the kernel's own per-call rows (sums within 1e-12 relative, everything else equal)."""
    import torch
    from mkz_mpc_path_follower_amd.ref_traj import fresh_score
    d = six
    fleet, dev = d["fleet"], d["fleet"].device
    ok0 = d["want"]["ok"]
    B = len(ok0)
    rng = np.random.default_rng(8)
    tol = 0.25
    score = fresh_score(B, dev)
    pid = np.where((d["pid"] >= 0) & (d["pid"] < len(d["paths"])), d["pid"], -1)
    states_np = [[] for _ in range(B)]
    states_gpu = [[] for _ in range(B)]
    sides = [[] for _ in range(B)]
    sum_abs = np.zeros((B, 2))
    for call in range(5):
        pose = d["pose"] + rng.normal(0, 0.2, d["pose"].shape) * (call > 0)
        if call == 2:
            pose[9, 1] = np.nan
        state = torch.zeros((B, 8), dtype=torch.float64, device=dev)
        state[:, 0:3] = torch.as_tensor(pose, device=dev)
        side = {}
        if call > 0:
            status = np.zeros(B, dtype=np.int32); status[7] = 1 if call == 2 else 0
            iters = rng.integers(2, 12, B).astype(np.int32)
            cmd = np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.4, 0.4, B)], 1)
            latch = np.zeros(B, dtype=np.uint8); latch[5] = call >= 3
            cmd[latch != 0] = (-1.0, 0.0)
            side = dict(status=torch.as_tensor(status, device=dev), iters=torch.as_tensor(iters, device=dev), cmd=torch.as_tensor(cmd, device=dev),
                        stop_latch=torch.as_tensor(latch, device=dev))
        o = fleet.track_score_batch(state, score=score, settle_tol=tol, **side)
        err = o["err"].cpu().numpy()
        w = numpy_errors(d["trs"], pose, pid)
        assert np.abs(np.abs(w["e_ct"][w["ok"]]) - tol).min() > 1e-6                # the settle index does not hinge on rounding
        for b in range(B):
            s_ = None if call == 0 else (status[b], iters[b], cmd[b, 0], cmd[b, 1], bool(latch[b]))
            sides[b].append(s_)
            states_np[b].append((w["e_ct"][b], w["e_near"][b], w["e_psi"][b]) if w["ok"][b] else None)
            states_gpu[b].append(tuple(err[b, :3]) if w["ok"][b] else None)
            if w["ok"][b]:
                sum_abs[b] += (abs(w["e_ct"][b]), abs(w["e_psi"][b]))
    got = score.cpu().numpy()
    assert np.isfinite(got).all()
    print("largest difference of a maximum to the accumulation of numpy's errors: %.3e" % max(R.maxima_diff(got[b], R.accumulate(R.fresh(), states_np[b], sides[b], tol)) for b in range(B)))
    for b in range(B):
        R.assert_record(got[b], R.accumulate(R.fresh(), states_np[b], sides[b], tol), BOUND_ACC, tag=("numpy", b), sum_slack=2 * BOUND_ACC * sum_abs[b].max())
        R.assert_record(got[b], R.accumulate(R.fresh(), states_gpu[b], sides[b], tol), 0.0, tag=("rows", b))
    f = dict(zip(R.FIELDS, got.T))
    assert f["latch_index"][5] == 2 and f["n_live"][5] == 2 and (np.delete(f["latch_index"], 5) == -1).all()
    assert f["n_nonopt"][7] == 1 and f["n_nonopt"].sum() == 1
    assert f["n_refused"][9] == 1 and f["n"][9] == 4 and f["n_live"][9] == 3 and (f["n_refused"][d["refused"]] == 5).all() and (f["n"][d["refused"]] == 0).all()
    assert (f["n"][ok0 & (np.arange(B) != 9)] == 5).all() and (f["settle_index"] > 0).any() and (f["settle_index"] == 0).any()


# ---------------------------------------------------------------- GPU, loops
def _download(r):
    return {k: r[k].cpu().numpy() for k in ("state", "cmd", "status", "latch")}


def _step_history(loop, steps):
    """the route the tests took before run(): step() plus downloads every period -> state [steps+1,B,8], cmd, status, iters, latch"""
    log = dict(state=[loop.sim.state.cpu().numpy().copy()], cmd=[], status=[], iters=[], latch=[])
    for _ in range(steps):
        o = loop.step()
        log["cmd"].append(o["cmd"].cpu().numpy().copy()); log["status"].append(o["status"].cpu().numpy().copy())
        log["iters"].append(o["iters"].cpu().numpy().copy()); log["latch"].append(loop.command_stop.cpu().numpy().copy())
        log["state"].append(loop.sim.state.cpu().numpy().copy())
    return {k: np.array(v) for k, v in log.items()}


def _check_run_against_steps(loop_run, loop_step, trs, steps, tol):
    """run(steps, history=True) against steps x step(): bit-identical histories; the score against the restatement on the downloaded history"""
    import torch
    fresh = loop_step.score.clone()
    r = loop_run.run(steps, history=True, settle_tol=tol)
    h = _step_history(loop_step, steps)
    torch.cuda.synchronize()
    assert torch.equal(loop_step.score, fresh)                                      # step() never scores
    g = _download(r)
    for k in ("state", "cmd", "status", "latch"):
        assert g[k].shape == h[k].shape and np.array_equal(g[k], h[k]), k
    got = r["score"].cpu().numpy()
    sm = loop_run.score_summary()
    recs, margin = [], np.inf
    for b, tr in enumerate(trs):
        rec, e = R.accumulate_history(tr, h["state"][:, b], h["cmd"][:, b], h["status"][:, b], h["iters"][:, b], h["latch"][:, b], tol)
        margin = min(margin, np.abs(np.abs(e["e_ct"]) - tol).min())
        recs.append((rec, e))
    print("settle_tol %.2f: the nearest |e_ct| of the history is %.3e m away" % (tol, margin))
    assert margin > 1e-6                                                            # precondition: the settle index does not hinge on rounding
    print("largest difference to the restatement: maxima %.3e, s_along of the last state %.3e m (s_along up to %.0f m)"
          % (max(R.maxima_diff(got[b], rec) for b, (rec, _e) in enumerate(recs)), max(abs(sm["s_along"][b] - e["s_along"][-1]) for b, (_r, e) in enumerate(recs)),
             max(e["s_along"][-1] for _r, e in recs)))
    for b, (rec, e) in enumerate(recs):
        R.assert_record(got[b], rec, BOUND_LOOP, tag=b, sum_slack=2 * BOUND_LOOP * max(np.abs(e["e_ct"]).sum(), np.abs(e["e_psi"]).sum()))
        s = S.summarize(trs[b], h["state"][:, b], h["cmd"][:, b], h["latch"][:, b])
        assert sm["n_live"][b] == s["n_live"] and abs(sm["max_dacc"][b] - s["max_dacc"]) <= BOUND_LOOP and abs(sm["max_ddf"][b] - s["max_ddf"]) <= BOUND_LOOP
        assert sm["latch_index"][b] == (-1 if s["t_stop"] is None else round(s["t_stop"] / 0.1))
        if tol == 0.5:
            assert sm["settle_index"][b] == round(s["t_converged"] / 0.1)
        assert abs(sm["rms_ect"][b] - np.sqrt((e["e_ct"] ** 2).mean())) <= BOUND_LOOP + 1e-12 and abs(sm["max_ect"][b] - s["ect"].max()) <= BOUND_LOOP
        assert abs(sm["s_along"][b] - e["s_along"][-1]) <= BOUND_LOOP
    assert (sm["n"] == steps + 1).all() and (sm["n_refused"] == 0).all()
    return sm, h


@pytest.mark.gpu
def test_mixed_fleet_run_equals_steps_and_scores_the_history():
    """the 18 vehicles of fleet_scenario for 60 periods: run() on one loop, 60 x step() on a second"""
    vs = F.vehicles()
    sm, h = _check_run_against_steps(F.make_loop(vs), F.make_loop(vs), [F.trajectory(v["path"]) for v in vs], F.STEPS, 0.5)
    for b, v in enumerate(vs):
        want = F.LATCH[v["kind"]][v["path"]]
        assert sm["latch_index"][b] == (-1 if want is None else want), (v["kind"], v["path"], sm["latch_index"][b])
    assert (sm["n_nonopt"] == 0).all() and (sm["latch_index"] >= 0).sum() == 6


def _frenet_loop(B=8):
    import torch
    from mkz_mpc_path_follower_amd import ClosedLoopFrenet
    from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory
    from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator
    arr, lat0, lon0 = S.path_arrays("path1_decimated.npz")
    grt = GPSRefTrajectory(arrays=arr, traj_horizon=H, traj_dt=0.2, lat0=lat0, lon0=lon0)
    tr = grt.get_global_trajectory_reference()
    rng = np.random.default_rng(42)
    idx = rng.integers(0, int(0.6 * len(tr)), B)
    sim = VehicleSimulator(B, X0=tr[idx, 4] + rng.uniform(-1, 1, B), Y0=tr[idx, 5] + rng.uniform(-1, 1, B), Psi0=tr[idx, 3] + rng.uniform(-0.2, 0.2, B))
    sim.state[:, 3] = torch.as_tensor(5.0 * rng.uniform(0.3, 1.0, B), dtype=torch.float64, device=sim.device)
    return ClosedLoopFrenet(grt, sim, H, 5.0), tr


@pytest.mark.gpu
def test_frenet_run_equals_steps_and_scores_the_history():
    """ClosedLoopFrenet, 8 vehicles on path1 at 5 m/s, 30 periods"""
    a, tr = _frenet_loop()
    b, _ = _frenet_loop()
    sm, _h = _check_run_against_steps(a, b, [tr] * 8, 30, 0.5)
    assert (sm["n_live"] == 30).all() and (sm["latch_index"] == -1).all()


@pytest.mark.gpu
def test_sweep_in_one_loop_equals_one_loop_per_setting():
    """8 weight settings x 3 start poses on path1, 40 periods: ONE loop of 24 vehicles with per-vehicle parameter records against 8 loops of 3 vehicles
    whose solver handle carries the setting -- the 24 score records are bit-identical (same kernel, same answer), so is the ranking"""
    import torch
    from mkz_mpc_path_follower_amd import BatchMPC, ClosedLoop
    from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory
    from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator
    arr, lat0, lon0 = S.path_arrays("path1_decimated.npz")
    grt = GPSRefTrajectory(arrays=arr, traj_horizon=H, traj_dt=0.2, lat0=lat0, lon0=lon0)
    tr = grt.get_global_trajectory_reference()
    rng = np.random.default_rng(6)
    nS, nV, steps = 8, 3, 40
    settings = np.array(S.WEIGHTS)[None, :].repeat(nS, 0)
    settings[:, [1, 2, 5]] *= np.exp(rng.uniform(-1.0, 1.0, (nS, 3)))                 # C_y, C_psi, C_ddf, log-uniform around the launch file's
    settings[:, 0] = settings[:, 1]                                                   # C_x = C_y, as in the launch file
    k = np.array([200, 900, 1500])
    start = np.stack([tr[k, 4] + np.array([0.6, -0.8, 0.3]), tr[k, 5] + np.array([-0.5, 0.4, 0.9]), tr[k, 3] + np.array([0.1, -0.15, 0.05])], 1)

    def sim_of(rows):
        sim = VehicleSimulator(len(rows), X0=rows[:, 0], Y0=rows[:, 1], Psi0=rows[:, 2])
        sim.state[:, 3] = 2.0
        return sim
    one = ClosedLoop(grt, sim_of(np.tile(start, (nS, 1))), N=H, target_vel=5.0, weights=S.WEIGHTS)
    par = one.mpc.problem_params(nS * nV)
    par[:, 0:8] = torch.as_tensor(np.repeat(settings, nV, axis=0), device=par.device)
    one.params = par
    big = one.run(steps)["score"].cpu().numpy()
    small = []
    for s in range(nS):
        loop = ClosedLoop(grt, sim_of(start), N=H, target_vel=5.0, mpc=BatchMPC(N=H, dtype=torch.float64, device=grt.device.index, weights=tuple(settings[s])))
        small.append(loop.run(steps)["score"].cpu().numpy())
    small = np.concatenate(small)
    assert np.array_equal(big, small)
    assert (big[:, 0] == steps + 1).all() and len(np.unique(big[:, 1])) == nS * nV    # the settings do differ
    rms = np.sqrt(big[:, 1] / big[:, 0]).reshape(nS, nV).mean(1)
    assert np.array_equal(np.argsort(rms), np.argsort(np.sqrt(small[:, 1] / small[:, 0]).reshape(nS, nV).mean(1)))
    grt.close()


@pytest.mark.gpu
def test_run_zero_scores_one_state_and_step_never_scores():
    import torch
    vs = F.vehicles()[:6]
    loop = F.make_loop(vs)
    fresh = loop.score.clone()
    want = np.zeros((6, 16)); want[:, 15] = -1
    assert np.array_equal(fresh.cpu().numpy(), want)
    for _ in range(3):
        loop.step()
    assert torch.equal(loop.score, fresh) and loop.track is None
    loop = F.make_loop(vs)
    r = loop.run(0)
    sc = r["score"].cpu().numpy()
    assert r["last"] is None and (sc[:, 0] == 1).all() and (sc[:, 8:15] == 0).all() and (sc[:, 15] == -1).all() and loop.k == 0
    loop.run(0)                                                                      # the record is no longer fresh: the initial state is not scored twice
    assert np.array_equal(loop.score.cpu().numpy(), sc)
    loop.run(2, score=False)
    assert np.array_equal(loop.score.cpu().numpy(), sc) and loop.k == 2
