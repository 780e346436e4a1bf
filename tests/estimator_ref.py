"""TEST INFRASTRUCTURE: numpy restatement of the state estimator (kmpc_estimate_batch), vectorised over the B vehicles and written from the
text of include/kmpc.h, not from the kernel: one call = one period of an extended Kalman filter on the solver's Euler bicycle, H = I, R diagonal,
four sequential scalar updates on the upper triangle of P.

estimate(rec, z, u, params, ...) -> (rec, est, innov, flags); predict / update_channel are the two halves, usable on their own (the CPU tests
compare them with a finite difference and with the textbook joint update).  Also here: the inputs the CPU and the GPU tests share
(single_call_case, consistency_case) so that both run the same numbers.
"""
import numpy as np

FIELDS = ("x", "y", "psi", "v", "pxx", "pxy", "pxpsi", "pxv", "pyy", "pypsi", "pyv", "ppsipsi", "ppsiv", "pvv", "count", "skipped")
PARAM_FIELDS = ("q_x", "q_y", "q_psi", "q_v", "r_x", "r_y", "r_psi", "r_v")
SKIP, INIT, RESET = (1, 2, 4, 8), 16, 32
L_A, L_B = 1.108, 1.742          # kmpc_config_default's (MKZMPCPathFollower.jl:33-34)
PI = 3.141592653589793
TRI = {}                         # (i, j), i <= j -> index into the 10 words of P
for _i in range(4):
    for _j in range(_i, 4):
        TRI[(_i, _j)] = len(TRI)


def wrap(a):
    """a inside [-pi, pi) unchanged, else fmod(a + pi, 2 pi) (+ 2 pi when negative) - pi: python's float % has the divisor's sign already"""
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inside = (a >= -PI) & (a < PI)
        return np.where(inside, a, (a + PI) % (2.0 * PI) - PI)


def tri_to_full(P10):
    """[B,10] -> [B,4,4] symmetric"""
    P10 = np.asarray(P10, dtype=np.float64)
    out = np.empty(P10.shape[:-1] + (4, 4))
    for (i, j), k in TRI.items():
        out[..., i, j] = out[..., j, i] = P10[..., k]
    return out


def full_to_tri(P):
    return np.stack([P[..., i, j] for (i, j) in TRI], axis=-1)


def model_step(xh, u, dt, L_a=L_A, L_b=L_B):
    """the solver's Euler step on xh [B,4] with u [B,2] -> (new xh, (s, c, sb)); psi, v on the right are the ones before the step"""
    x, y, psi, v = (xh[:, i] for i in range(4))
    beta = np.arctan(L_b / (L_a + L_b) * np.tan(u[:, 1]))
    s, c, sb = np.sin(psi + beta), np.cos(psi + beta), np.sin(beta)
    vn = v + dt * u[:, 0]
    new = np.stack([x + dt * (v * c), y + dt * (v * s), wrap(psi + dt * (v / L_b * sb)), np.where(vn < 0.0, 0.0, vn)], axis=1)
    return new, (s, c, sb)


def jacobian(xh, u, dt, L_a=L_A, L_b=L_B):
    """F [B,4,4] = I + the five entries of the header"""
    v = xh[:, 3]
    _, (s, c, sb) = model_step(xh, u, dt, L_a, L_b)
    F = np.tile(np.eye(4), (len(xh), 1, 1))
    F[:, 0, 2], F[:, 0, 3], F[:, 1, 2], F[:, 1, 3], F[:, 2, 3] = -(dt * (v * s)), dt * c, dt * (v * c), dt * s, dt * (sb / L_b)
    return F


def predict(xh, P10, u, q2, dt, L_a=L_A, L_b=L_B):
    """-> (xh, P10) after the step; only the upper triangle is formed, sums left to right as the header has them"""
    v = xh[:, 3]
    new, (s, c, sb) = model_step(xh, u, dt, L_a, L_b)
    fxp, fxv, fyp, fyv, fpv = -(dt * (v * s)), dt * c, dt * (v * c), dt * s, dt * (sb / L_b)
    pxx, pxy, pxs, pxv, pyy, pys, pyv, pss, psv, pvv = (P10[:, k] for k in range(10))
    Axx, Axy = pxx + fxp * pxs + fxv * pxv, pxy + fxp * pys + fxv * pyv
    Axs, Axv = pxs + fxp * pss + fxv * psv, pxv + fxp * psv + fxv * pvv
    Ayy, Ays, Ayv = pyy + fyp * pys + fyv * pyv, pys + fyp * pss + fyv * psv, pyv + fyp * psv + fyv * pvv
    Ass, Asv = pss + fpv * psv, psv + fpv * pvv
    out = np.stack([Axx + fxp * Axs + fxv * Axv + q2[:, 0], Axy + fyp * Axs + fyv * Axv, Axs + fpv * Axv, Axv,
                    Ayy + fyp * Ays + fyv * Ayv + q2[:, 1], Ays + fpv * Ayv, Ayv,
                    Ass + fpv * Asv + q2[:, 2], Asv,
                    pvv + q2[:, 3]], axis=1)
    return new, out


def update_channel(xh, P10, c, z_c, r2_c, gate=0.0):
    """one scalar update of channel c -> (xh, P10, innov [B], skipped [B] bool)"""
    with np.errstate(all="ignore"):
        nu = z_c - xh[:, c]
        if c == 2:
            nu = wrap(nu)
        S = P10[:, TRI[(c, c)]] + r2_c
        skip = ~np.isfinite(z_c) | ~((S > 0.0) & np.isfinite(S))
        if gate > 0.0:
            skip = skip | (nu * nu > gate * gate * S)
        col = np.stack([P10[:, TRI[(min(a, c), max(a, c))]] for a in range(4)], axis=1)    # column c of P before this channel
        K = col / S[:, None]
        xn = xh + K * nu[:, None]
        Pn = P10.copy()
        for (a, b), k in TRI.items():
            Pn[:, k] = P10[:, k] - K[:, a] * col[:, b]
        innov = nu / np.sqrt(S)
    sk = skip[:, None]
    return np.where(sk, xh, xn), np.where(sk, P10, Pn), np.where(skip, 0.0, innov), skip


def estimate(rec, z, u, params, dt=0.1, L_a=L_A, L_b=L_B, gate=0.0):
    """rec [B,16], z [B,4], u [B,2], params [B,8] -> (rec after the call, est [B,4], innov [B,4], flags [B] int32)"""
    rec, z, u, params = (np.array(a, dtype=np.float64, copy=True) for a in (rec, z, u, params))
    B = len(rec)
    q2, r2 = params[:, 0:4] * params[:, 0:4], params[:, 4:8] * params[:, 4:8]
    first = rec[:, 14] == 0.0
    zfin = np.isfinite(z)
    # every vehicle goes through predict + update; the first-call ones are overwritten afterwards (numpy computes both arms, as a select would)
    with np.errstate(all="ignore"):
        xh, P10 = predict(rec[:, 0:4], rec[:, 4:14], u, q2, dt, L_a, L_b)
        innov, flags, nskip = np.zeros((B, 4)), np.zeros(B, dtype=np.int32), np.zeros(B)
        for c in range(4):
            xh, P10, innov[:, c], sk = update_channel(xh, P10, c, z[:, c], r2[:, c], gate)
            flags |= np.where(sk, SKIP[c], 0).astype(np.int32)
            nskip += sk
        xh[:, 2] = wrap(xh[:, 2])
        xh[:, 3] = np.where(xh[:, 3] < 0.0, 0.0, xh[:, 3])
        out = np.concatenate([xh, P10, (rec[:, 14] + 1.0)[:, None], (rec[:, 15] + nskip)[:, None]], axis=1)
    bad = ~np.isfinite(out).all(1)
    flags = np.where(bad, flags | RESET, flags).astype(np.int32)
    # first call on a fresh record
    init = first & zfin.all(1)
    fresh_stays = first & ~zfin.all(1)
    first_rec = np.zeros((B, 16))
    first_rec[:, 0:4] = z
    for c in range(4):
        first_rec[:, 4 + TRI[(c, c)]] = r2[:, c]
    first_rec[:, 14] = 1.0
    out = np.where(init[:, None], first_rec, out)
    flags = np.where(init, INIT, flags)
    flags = np.where(fresh_stays, ((~zfin) * np.array(SKIP)).sum(1), flags).astype(np.int32)
    to_fresh = fresh_stays | (bad & ~first)
    out = np.where(to_fresh[:, None], 0.0, out)
    est = np.where(to_fresh[:, None], z, out[:, 0:4])
    innov = np.where((first | to_fresh)[:, None], 0.0, innov)
    return out, est, innov, flags


# ---------------------------------------------------------------- inputs shared by tests/test_estimator_ref.py (CPU) and tests/test_estimator.py (GPU)
def random_spd(rng, B, scale=(0.3, 0.3, 0.03, 0.2)):
    """[B,4,4] covariances with standard deviations around `scale` and full correlations"""
    A = rng.normal(0, 1, (B, 4, 4))
    P = A @ A.transpose(0, 2, 1) / 4.0 + 0.05 * np.eye(4)
    d = np.asarray(scale) * rng.uniform(0.5, 2.0, (B, 4))
    return P * d[:, :, None] * d[:, None, :]


SINGLE_SEED, SINGLE_B, SINGLE_GATE = 31, 300, 3.0


def single_call_case():
    """B = 300 records in mid-run with SPD P, x, y within +-500 m, psi over the whole circle, a tenth standing, and the groups of the GPU test:
    [0, 20) psi-hat and z_psi on opposite sides of +-pi; [20, 40) one NaN channel (five vehicles per channel); [40, 60) an 8 sigma outlier in one
    channel under gate = 3 (five per channel); [60, 70) fresh records, of which 68 and 69 get a non-finite measurement.
    The measurement is pred + L n with L the Cholesky factor of P_pred + R: the sequential updates' normalised innovations are then exactly n
    (whitening in the order x, y, psi, v IS the Cholesky factorisation), so |n| <= 2 passes the gate and n_c = +-8 is an 8 sigma outlier of
    channel c as the filter sees it.  -> dict(rec, z, u, params, gate, dt, n)"""
    rng = np.random.default_rng(SINGLE_SEED)
    B = SINGLE_B
    rec = np.zeros((B, 16))
    rec[:, 0:2] = rng.uniform(-500, 500, (B, 2))
    rec[:, 2] = rng.uniform(-np.pi, np.pi, B)
    rec[:, 3] = np.where(rng.random(B) < 0.1, 0.0, rng.uniform(0, 20, B))
    rec[0:70, 3] = rng.uniform(2, 10, 70)                                         # the special groups all move
    rec[:, 4:14] = full_to_tri(random_spd(rng, B))
    rec[:, 14] = rng.integers(1, 500, B)
    rec[:, 15] = rng.integers(0, 7, B)
    params = np.empty((B, 8))
    params[:, 0:4] = np.array([0.02, 0.02, 0.01, 0.1]) * rng.uniform(0.5, 2.0, (B, 4))
    params[:, 4:8] = np.array([0.2, 0.2, 0.02, 0.1]) * rng.uniform(0.5, 2.0, (B, 4))
    u = np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.5, 0.5, B)], 1)               # standing vehicles brake or pull away: the floor at v = 0
    u[0:20, 1] = 0.0                                                                  # no steering: the predict leaves psi-hat where it is
    rec[0:20, 2] = np.where(np.arange(20) % 2 == 0, 1.0, -1.0) * (PI - 1e-6)
    n = np.clip(rng.normal(0, 1, (B, 4)), -2.0, 2.0)
    for k in range(20):
        n[40 + k, k % 4] = 8.0 if k % 8 < 4 else -8.0
    pred, Ppred = predict(rec[:, 0:4], rec[:, 4:14], u, params[:, 0:4] ** 2, 0.1)
    S = tri_to_full(Ppred)
    S[:, range(4), range(4)] += params[:, 4:8] ** 2
    delta = np.einsum("bij,bj->bi", np.linalg.cholesky(S), n)
    flip = np.sign(delta[0:20, 2]) != np.sign(rec[0:20, 2])                           # push the heading measurement across the cut
    n[0:20][flip] *= -1.0
    delta[0:20][flip] *= -1.0
    z = pred + delta
    z[:, 2] = wrap(z[:, 2])
    for k in range(20):
        z[20 + k, k % 4] = np.nan
    rec[60:70] = 0.0
    z[68, 1] = np.nan
    z[69, 3] = np.inf
    return dict(rec=rec, z=z, u=u, params=params, gate=SINGLE_GATE, dt=0.1, n=n)


CONS_SEED, CONS_B, CONS_STEPS = 47, 256, 100
CONS_Q, CONS_R = (0.02, 0.02, 0.01, 0.1), (0.2, 0.2, 0.02, 0.1)


def consistency_case():
    """256 vehicles x 100 periods, open loop: the truth from the same Euler model with process noise N(0, q^2) and constant inputs per vehicle,
    measurements with sigma = CONS_R, all drawn here with a fixed seed -> dict(truth [K,B,4], z [K,B,4], u [B,2], params [B,8]); z[0]
    initialises the filter, so 100 calls are 99 updates, and z[k] is the measurement of truth[k].  Speeds start at 4..12 m/s with |acc| <= 0.3 so that no vehicle reaches the
    floor at v = 0, where the truth's noise would stop being Gaussian."""
    rng = np.random.default_rng(CONS_SEED)
    B, K = CONS_B, CONS_STEPS
    q, r = np.array(CONS_Q), np.array(CONS_R)
    x = np.stack([rng.uniform(-500, 500, B), rng.uniform(-500, 500, B), rng.uniform(-np.pi, np.pi, B), rng.uniform(4, 12, B)], 1)
    u = np.stack([rng.uniform(-0.3, 0.3, B) * 0.1, rng.uniform(-0.1, 0.1, B)], 1)
    truth, z = np.empty((K, B, 4)), np.empty((K, B, 4))
    for k in range(K):
        if k:
            x, _ = model_step(x, u, 0.1)
            x = x + q * rng.normal(0, 1, (B, 4))
            x[:, 2] = wrap(x[:, 2])
        truth[k] = x
        z[k] = x + r * rng.normal(0, 1, (B, 4))
        z[k, :, 2] = wrap(z[k, :, 2])
    assert truth[:, :, 3].min() > 1.0
    return dict(truth=truth, z=z, u=u, params=np.tile(np.concatenate([q, r]), (B, 1)))


def run_recursion(z, u, params, gate=0.0, dt=0.1):
    """the restatement over z [K,B,4] from fresh records -> dict(rec [K,B,16], est, innov [K,B,4], flags [K,B])"""
    K1, B = z.shape[0], z.shape[1]
    rec = np.zeros((B, 16))
    out = dict(rec=np.empty((K1, B, 16)), est=np.empty((K1, B, 4)), innov=np.empty((K1, B, 4)), flags=np.empty((K1, B), dtype=np.int32))
    for k in range(K1):
        rec, out["est"][k], out["innov"][k], out["flags"][k] = estimate(rec, z[k], u, params, dt=dt, gate=gate)
        out["rec"][k] = rec
    return out
