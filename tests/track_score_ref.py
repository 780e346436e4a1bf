"""numpy / plain-Python restatement of the tracking score (test helper): what kmpc_track_score_batch / _fleet compute per call and accumulate per vehicle.

Per state (include/kmpc.h, "tracking errors on the recorded paths"):
  e_ct     signed distance to the polyline -- scenario.cross_track's distance and segment, the sign of d x w on that segment (>= 0 positive: left of travel)
  e_near   distance to the nearest recorded sample -- compute_path_errors of the reference's scripts/analysis/plot_path_tracking_error.py:21-34
  e_psi    fix_heading(psi_path[closest] - psi) (:36-43, :161)
  s_along  cdist[seg] + s (cdist[seg+1] - cdist[seg])
Per vehicle: `accumulate`, the record of ref_traj.SCORE_FIELDS as a plain loop over a history; it must agree with scenario.summarize on the fields that has.
"""
import numpy as np

import scenario as S

FIELDS = ("n", "sum_ect2", "max_ect", "sum_epsi2", "max_epsi", "max_enear", "settle_index", "n_refused",
          "n_live", "n_nonopt", "sum_iters", "max_dacc", "max_ddf", "last_acc", "last_df", "latch_index")
COUNTS = ("n", "settle_index", "n_refused", "n_live", "n_nonopt", "sum_iters", "latch_index")   # exact
MAXIMA = ("max_ect", "max_epsi", "max_enear", "max_dacc", "max_ddf", "last_acc", "last_df")
SUMS = ("sum_ect2", "sum_epsi2")


def segment_point(traj_xy, seg, x, y):
    """distance of (x[i], y[i]) to segment seg[i] -> seg[i] + 1 of the polyline, the clamped parameter s and d x w (scenario.cross_track's formulation)"""
    P, Q = traj_xy[seg], traj_xy[np.asarray(seg) + 1]
    d = Q - P
    w = np.stack([x - P[:, 0], y - P[:, 1]], 1)
    s = np.clip((w * d).sum(1) / np.maximum((d ** 2).sum(1), 1e-18), 0.0, 1.0)
    e = np.sqrt(((w - s[:, None] * d) ** 2).sum(1))
    return e, s, d[:, 0] * w[:, 1] - d[:, 1] * w[:, 0]


def nearest_sample(traj_xy, x, y):
    """-> (distance to the nearest sample, its index: first occurrence) with the arithmetic of the waypoint helper's argmin"""
    idx = np.empty(len(x), dtype=np.int64)
    dist = np.empty(len(x))
    for i, (xi, yi) in enumerate(zip(x, y)):
        d2 = (traj_xy[:, 0] - xi) ** 2 + (traj_xy[:, 1] - yi) ** 2
        idx[i] = int(np.argmin(d2))
        dist[i] = np.sqrt(d2[idx[i]])
    return dist, idx


def fix_heading(p):
    """plot_path_tracking_error.py:36-43, not in place"""
    p = np.asarray(p, dtype=np.float64)
    cands = np.stack([p, p + 2 * np.pi, p - 2 * np.pi], 0)
    return cands[np.argmin(np.fabs(cands), axis=0), np.arange(len(p))]


def errors(traj, x, y, psi):
    """traj [M,7] (t, lat, lon, psi, X, Y, cdist); x, y, psi arrays -> dict e_ct, e_near, e_psi, s_along, seg, closest, e_abs (unsigned, cross_track's)"""
    x, y, psi = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (x, y, psi))
    xy = traj[:, 4:6]
    e_abs, seg = S.cross_track(xy, x, y)
    e, s, cross = segment_point(xy, seg, x, y)
    e_near, closest = nearest_sample(xy, x, y)
    return dict(e_abs=e_abs, e_ct=np.where(cross >= 0.0, e, -e), e_near=e_near, e_psi=fix_heading(traj[closest, 3] - psi),
                s_along=traj[seg, 6] + s * (traj[seg + 1, 6] - traj[seg, 6]), seg=seg, closest=closest, cross=cross)


def fresh():
    r = dict.fromkeys(FIELDS, 0.0)
    r["latch_index"] = -1.0
    return r


def accumulate(rec, states, sides, settle_tol):
    """one vehicle: rec (dict, updated and returned) over states[j] = (e_ct, e_near, e_psi) or None (refused) and sides[j] = None (geometry only) or
    (status, iters, acc, df, latched)"""
    for st, side in zip(states, sides):
        if st is None:
            rec["n_refused"] += 1
            continue
        e_ct, e_near, e_psi = (float(v) for v in st)
        if abs(e_ct) >= settle_tol:
            rec["settle_index"] = rec["n"] + 1
        rec["n"] += 1
        rec["sum_ect2"] += e_ct * e_ct
        rec["max_ect"] = max(rec["max_ect"], abs(e_ct))
        rec["sum_epsi2"] += e_psi * e_psi
        rec["max_epsi"] = max(rec["max_epsi"], abs(e_psi))
        rec["max_enear"] = max(rec["max_enear"], e_near)
        if side is None:
            continue
        status, iters, acc, df, latched = side
        if latched:
            if rec["latch_index"] < 0:
                rec["latch_index"] = rec["n_live"]
            continue
        rec["n_live"] += 1
        rec["n_nonopt"] += int(status != 0)
        rec["sum_iters"] += int(iters)
        rec["max_dacc"] = max(rec["max_dacc"], abs(float(acc) - rec["last_acc"]))
        rec["max_ddf"] = max(rec["max_ddf"], abs(float(df) - rec["last_df"]))
        rec["last_acc"], rec["last_df"] = float(acc), float(df)
    return rec


def accumulate_history(traj, state, cmd, status, iters, latch, settle_tol):
    """one vehicle of a run: state [T+1,>=3] (the state before the first period first), cmd [T,2], status, iters, latch [T] -> (record, errors dict)"""
    e = errors(traj, state[:, 0], state[:, 1], state[:, 2])
    states = list(zip(e["e_ct"], e["e_near"], e["e_psi"]))
    sides = [None] + [(status[k], iters[k], cmd[k, 0], cmd[k, 1], bool(latch[k])) for k in range(len(cmd))]
    return accumulate(fresh(), states, sides, settle_tol), e


def maxima_diff(got, want):
    """largest difference over the maxima and the kept command (what `bound` of assert_record is compared with)"""
    g = dict(zip(FIELDS, (float(v) for v in got)))
    return max(abs(g[k] - want[k]) for k in MAXIMA)


def assert_record(got, want, bound, tag="", sum_slack=0.0):
    """got: 16 numbers in FIELDS order; want: dict.  Counts and indices exact, maxima (and the kept command) within `bound`, sums within 1e-12 relative
    (+ sum_slack, absolute: what errors that themselves differ by `bound` per state may add -- 2 * bound * sum |e|)."""
    g = dict(zip(FIELDS, (float(v) for v in got)))
    for k in COUNTS:
        assert g[k] == want[k], (tag, k, g[k], want[k])
    for k in MAXIMA:
        assert abs(g[k] - want[k]) <= bound, (tag, k, g[k], want[k])
    for k in SUMS:
        assert abs(g[k] - want[k]) <= 1e-12 * abs(want[k]) + sum_slack, (tag, k, g[k], want[k])
