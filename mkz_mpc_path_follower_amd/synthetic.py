"""Seeded synthetic (x0, path-segment) batches for tests and bench.py.

The reference ships no benchmark inputs.  The distribution follows SURVEY.md section 8(d):
reference segments are circular arcs with the curvature / speed range of the recorded
paths (paths/*.mat: |kappa| <= 0.10 1/m, v <= 11.3 m/s), sampled the way
scripts/gps_utils/ref_gps_traj.py:172-179 samples waypoints (arclength v_target*dt*k),
initial states are perturbed poses on the arc, and a 5 % "hard" stratum holds the
launch/sim_path_follow.launch:23-25 style cases (3 m lateral offset; standing start).
"""
import numpy as np

SEED_BASE = 20180620


def make_batch(B, N, cfg_id=2, dt=0.2, hard_frac=0.05, dtype=np.float64, seed=None):
    """returns dict z0[B,4], ref[B,N+1,3], v_target[B], u_prev[B,2] (acc, steer), hard[B] (bool)"""
    rng = np.random.default_rng(SEED_BASE + cfg_id if seed is None else seed)
    kappa = rng.uniform(-0.09, 0.09, B)
    v_t = rng.uniform(2.0, 11.0, B)
    th0 = rng.uniform(-np.pi, np.pi, B)
    e_y = rng.normal(0.0, 0.5, B)
    e_psi = rng.normal(0.0, 0.05, B)
    v0 = np.clip(v_t + rng.normal(0.0, 1.0, B), 0.0, 20.0)
    acc_prev = rng.uniform(-0.5, 0.5, B)
    df_prev = np.clip(np.arctan(2.85 * kappa) + rng.normal(0.0, 0.01, B), -0.5, 0.5)
    hard = rng.uniform(size=B) < hard_frac
    kind = rng.uniform(size=B) < 0.5
    sign = np.where(rng.uniform(size=B) < 0.5, -1.0, 1.0)
    # hard stratum: standing start (v0 = 0, previous accel 0) or 3 m lateral offset
    rest = hard & kind
    far = hard & ~kind
    v0 = np.where(rest, 0.0, v0)
    acc_prev = np.where(rest, 0.0, acc_prev)
    e_y = np.where(far, 3.0 * sign, e_y)
    # keep every instance feasible: the first-step rate limit (|acc_1 - acc_prev| <= 0.15) must leave
    # room for v_2 = v0 + dt*acc_1 >= 0 (a standing car whose last command was hard braking has no
    # feasible input in the reference NLP; that case is exercised by an explicit edge-case test)
    acc_prev = np.maximum(acc_prev, -v0 / dt - 0.10)

    s = v_t[:, None] * dt * np.arange(N + 1)[None, :]
    ks = kappa[:, None] * s
    small = np.abs(kappa)[:, None] < 1e-9
    ksafe = np.where(small, 1.0, kappa[:, None])
    xr = np.where(small, s * np.cos(th0)[:, None], (np.sin(th0[:, None] + ks) - np.sin(th0)[:, None]) / ksafe)
    yr = np.where(small, s * np.sin(th0)[:, None], -(np.cos(th0[:, None] + ks) - np.cos(th0)[:, None]) / ksafe)
    pr = th0[:, None] + ks
    ref = np.stack([xr, yr, pr], axis=-1)
    z0 = np.stack([-e_y * np.sin(th0), e_y * np.cos(th0), th0 + e_psi, v0], axis=-1)
    u_prev = np.stack([acc_prev, df_prev], axis=-1)
    return dict(z0=z0.astype(dtype), ref=ref.astype(dtype), v_target=v_t.astype(dtype),
                u_prev=u_prev.astype(dtype), hard=hard)


def straight_line_case(N, v0=0.0, y0=0.0, psi0=0.0, v_ref=15.0, dt=0.2):
    """The module-load problem of MKZMPCPathFollower.jl:36-39,110-113 (BASELINE config 1 at N=8)."""
    ref = np.zeros((1, N + 1, 3))
    ref[0, :, 0] = v_ref * dt * np.arange(N + 1)
    z0 = np.array([[0.0, y0, psi0, v0]])
    return dict(z0=z0, ref=ref, v_target=np.array([v_ref]), u_prev=np.zeros((1, 2)), hard=np.array([False]))


def _feasible_acc_prev(acc_prev, v0, dt, v_max=20.0):
    """keep the first-step rate interval (|acc_1 - acc_prev| <= 0.15) compatible with 0 <= v0 + dt * acc_1 <= v_max (see make_batch)"""
    return np.minimum(np.maximum(acc_prev, -v0 / dt - 0.10), (v_max - v0) / dt + 0.10)


def make_ood_batch(B, N, seed, paths=None, dt=0.2, dtype=np.float64):
    """Out-of-distribution batch (tools/ood_sweep.py, tests/test_gpu_parity.py): far wider than make_batch on every axis the iteration's
    rules were tuned on -- heading error N(0, 0.3 rad), lateral error U(-4, 4) m, initial speed U(0, 20) m/s INDEPENDENT of the reference's speed, previous
    command anywhere in the input box.  Two reference families, half of the batch each (all of it family A when `paths` is None):
      A  circular arcs with |kappa| <= 0.2 1/m (twice the recorded paths' range) at 0.5 ... 11 m/s;
      B  time-mode windows of the recorded paths (ref_gps_traj.py:186-195: N + 1 samples of the recorded x, y, psi at t_i + 0.2 h, so the spacing follows
         the recorded speed profile, 0.5 ... 11 m/s, including windows that run into the path's end, where np.interp clamps and the waypoints coincide),
         `paths` = list of dicts with t, x, y, psi (the fixtures tests/golden/path*_decimated.npz); psi is unwrapped against the vehicle's heading as the
         helper does (:204-218).
    returns the make_batch dict + family[B] (0 = A, 1 = B)"""
    rng = np.random.default_rng(seed)
    fam = (rng.uniform(size=B) < 0.5).astype(np.int64) if paths else np.zeros(B, dtype=np.int64)
    e_y = rng.uniform(-4.0, 4.0, B)
    e_psi = rng.normal(0.0, 0.3, B)
    v0 = rng.uniform(0.0, 20.0, B)
    acc_prev = _feasible_acc_prev(rng.uniform(-1.0, 1.0, B), v0, dt)
    df_prev = rng.uniform(-0.5, 0.5, B)
    # family A
    kappa = rng.uniform(-0.2, 0.2, B)
    v_t = rng.uniform(0.5, 11.0, B)
    th0 = rng.uniform(-np.pi, np.pi, B)
    s = v_t[:, None] * dt * np.arange(N + 1)[None, :]
    ks = kappa[:, None] * s
    small = np.abs(kappa)[:, None] < 1e-9
    ksafe = np.where(small, 1.0, kappa[:, None])
    xr = np.where(small, s * np.cos(th0)[:, None], (np.sin(th0[:, None] + ks) - np.sin(th0)[:, None]) / ksafe)
    yr = np.where(small, s * np.sin(th0)[:, None], -(np.cos(th0[:, None] + ks) - np.cos(th0)[:, None]) / ksafe)
    pr = th0[:, None] + ks
    x0, y0, h0 = np.zeros(B), np.zeros(B), th0.copy()
    if paths:
        which = rng.integers(0, len(paths), B)
        for k, P in enumerate(paths):
            m = np.where((fam == 1) & (which == k))[0]
            if len(m) == 0:
                continue
            t, px, py, pp = (np.asarray(P[c], dtype=np.float64) for c in ("t", "x", "y", "psi"))
            i0 = rng.integers(0, len(t), len(m))
            grid = t[i0][:, None] + dt * np.arange(N + 1)[None, :]
            xr[m] = np.interp(grid.ravel(), t, px).reshape(grid.shape)
            yr[m] = np.interp(grid.ravel(), t, py).reshape(grid.shape)
            pr[m] = np.interp(grid.ravel(), t, pp).reshape(grid.shape)          # interpolated BEFORE unwrapping, as the reference does (Q8)
            x0[m], y0[m], h0[m] = px[i0], py[i0], pp[i0]
            v_t[m] = 1.0                                                         # des_speed of the launch file; C_v = 0
    psi0 = h0 + e_psi
    if paths:   # the helper's wrap fix (:204-218), vectorised: candidates p, p + 2 pi, p - 2 pi closest to the vehicle's heading, for the rows that fail its two checks
        m = np.where(fam == 1)[0]
        bad = (np.abs(np.diff(pr[m], axis=1)).max(1) >= np.pi) | (np.abs(pr[m] - psi0[m, None]).max(1) >= np.pi)
        mm = m[bad]
        c = np.stack([pr[mm], pr[mm] + 2 * np.pi, pr[mm] - 2 * np.pi], -1)
        pr[mm] = np.take_along_axis(c, np.abs(c - psi0[mm, None, None]).argmin(-1)[..., None], -1)[..., 0]
    ref = np.stack([xr, yr, pr], axis=-1)
    z0 = np.stack([x0 - e_y * np.sin(h0), y0 + e_y * np.cos(h0), psi0, v0], axis=-1)
    u_prev = np.stack([acc_prev, df_prev], axis=-1)
    return dict(z0=z0.astype(dtype), ref=ref.astype(dtype), v_target=v_t.astype(dtype), u_prev=u_prev.astype(dtype), hard=np.zeros(B, dtype=bool), family=fam)


# ---- per-problem weights and limits (BatchMPC.solve(..., params=), kmpc_solve_batch_params) -----------------------------------------
PARAM_BASE = np.array([9.0, 9.0, 10.0, 1.0, 100.0, 1000.0, 1.0, 1.0])
LIMIT_NAMES = ("steer_max", "steer_dmax", "a_max", "a_dmax", "v_min", "v_max")   # record slots 8 ... 13, in this order


def make_param_sets(G, seed, model=0):
    """G seeded (weights[8], limits dict) pairs: weights within a decade either side of PARAM_BASE (C_v, C_acc, C_df zero a quarter of the time; pose and
    rate weights never), limits inside ranges that keep make_batch's feasibility argument (|acc_prev| <= 0.5 < a_max, first-step margin 0.10 < a_dmax *
    dt_control) and the start point's 0.6 a_max < a_dmax."""
    rng = np.random.default_rng(seed)
    out = []
    for g in range(G):
        w = PARAM_BASE * 10.0 ** rng.uniform(-1, 1, 8)
        z = rng.uniform(size=8) < 0.25
        z[[0, 1, 2, 4, 5]] = False          # pose and rate weights are never zero
        w[z] = 0.0
        if model == 1:
            w[0] = 0.0                      # the Frenet module has no x slot
        lim = dict(steer_max=rng.uniform(0.35, 0.5), steer_dmax=rng.uniform(0.3, 0.5), a_max=rng.uniform(0.8, 1.0),
                   a_dmax=rng.uniform(1.2, 1.5), v_min=0.0, v_max=rng.uniform(9.0, 20.0))
        out.append((w, lim))
    return out


def param_records(sets, B, dtype=np.float64):
    """records [B,16] in the layout of include/kmpc.h: problem i carries set i % len(sets)"""
    rec = np.zeros((B, 16))
    for i in range(B):
        w, lim = sets[i % len(sets)]
        rec[i, 0:8] = w
        rec[i, 8:14] = [lim[k] for k in LIMIT_NAMES]
    return rec.astype(dtype)


def apply_param_sets(batch, sets, v_col=3):
    """problem i of `batch` (make_batch dict, or any dict with z0) gets set i % G: its v0 is lowered to min(v0, v_max_i - 0.5) in place; returns records [B,16]"""
    B = len(batch["z0"])
    rec = param_records(sets, B, batch["z0"].dtype)
    batch["z0"][:, v_col] = np.minimum(batch["z0"][:, v_col], rec[:, 13] - 0.5)
    return rec
