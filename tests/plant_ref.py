"""TEST INFRASTRUCTURE: numpy restatements of the per-vehicle plant (kmpc_sim_advance_plant) and of the measurement stage (kmpc_sense_batch),
written from include/kmpc.h and oracle/vehicle_sim.py, not from the kernels.

update_plant: oracle.vehicle_sim.update_vehicle_model with the module constants replaced by a row per vehicle (KMPC_PLANT_* order) and the command
switched from cmd_held to cmd after cmd_delay model updates.  With DEFAULT_ROW and no delay it equals the oracle bit for bit
(tests/test_plant_sensor_ref.py).
philox4x32_10 / normals / sense: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) in Python
integers, checked against Random123's published known answers, then Box-Muller as the header specifies it.
"""
import numpy as np

from oracle import vehicle_sim as V

FIELDS = ("lf", "lr", "m", "Iz", "C_alpha_f", "C_alpha_r", "k_acc", "k_df")
DEFAULT_ROW = np.array([V.LF, V.LR, V.MASS, V.IZ, V.C_ALPHA_F, V.C_ALPHA_R, V.KP, V.KP])
SENSOR_FIELDS = ("sigma_x", "sigma_y", "sigma_psi", "sigma_v", "bias_x", "bias_y", "bias_psi", "bias_v")


def update_plant(state, cmd, plant, n_updates=1, cmd_delay=None, cmd_held=None, disc_steps=V.DISC_STEPS, slip=None):
    """-> (state [B,8], cmd_held [B,2] after the call).  slip: a list that receives max |tan alpha_f|, |tan alpha_r| over moving sub-steps"""
    s = np.array(state, dtype=np.float64, copy=True)
    B = len(s)
    X, Y, psi, vx, vy, wz, acc, df = (s[:, i].copy() for i in range(8))
    cmd = np.asarray(cmd, dtype=np.float64)
    lf, lr, m, Iz, Cf, Cr, k_acc, k_df = (np.asarray(plant, dtype=np.float64)[:, i] for i in range(8))
    inv_m, inv_Iz = 1.0 / m, 1.0 / Iz
    d = np.zeros(B, dtype=np.int64) if cmd_delay is None else np.clip(np.asarray(cmd_delay, dtype=np.int64), 0, n_updates)
    held = cmd if cmd_held is None else np.asarray(cmd_held, dtype=np.float64)
    deltaT = V.DT_MODEL / disc_steps
    worst = 0.0
    for it in range(n_updates * disc_steps):
        old = it < d * disc_steps
        acc_des, df_des = np.where(old, held[:, 0], cmd[:, 0]), np.where(old, held[:, 1], cmd[:, 1])
        moving = np.fabs(vx) > 1e-6
        if slip is not None and moving.any():
            with np.errstate(all="ignore"):
                worst = max(worst, np.abs((vy + lf * wz) / vx)[moving].max(), np.abs((vy - lf * wz) / vx)[moving].max())
        alpha_f = np.where(moving, df - np.arctan2(vy + lf * wz, vx), 0.0)
        alpha_r = np.where(moving, -np.arctan2(vy - lf * wz, vx), 0.0)          # lf, as in the reference
        Fyf = Cf * alpha_f
        Fyr = Cr * alpha_r
        vx_n = np.maximum(0.0, vx + deltaT * (acc + wz * vy))                   # no Fyf sin(df) / m term, as in the reference
        fwd = vx_n > 1e-6
        vy_n = np.where(fwd, vy + deltaT * (inv_m * (Fyf * np.cos(df) + Fyr) - wz * vx), 0.0)
        wz_n = np.where(fwd, wz + deltaT * (inv_Iz * (lf * Fyf * np.cos(df) - lr * Fyr)), 0.0)
        psi_n = psi + deltaT * wz
        X_n = X + deltaT * (vx * np.cos(psi) - vy * np.sin(psi))
        Y_n = Y + deltaT * (vx * np.sin(psi) + vy * np.cos(psi))
        X, Y = X_n, Y_n
        psi = (psi_n + np.pi) % (2.0 * np.pi) - np.pi
        vx, vy, wz = vx_n, vy_n, wz_n
        acc = k_acc * (acc_des - acc) * deltaT + acc
        df = k_df * (df_des - df) * deltaT + df
    if slip is not None:
        slip.append(worst)
    return np.stack([X, Y, psi, vx, vy, wz, acc, df], axis=1), cmd.copy()


M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: four uint32, key: two uint32 (Python ints) -> four uint32"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def normals(seed, gid, period):
    """the four normals of vehicle `gid` in period `period` (include/kmpc.h, kmpc_sense_batch) -> [4] for x, y, psi, v"""
    w = philox4x32_10((gid & M32, (gid >> 32) & M32, period & M32, (period >> 32) & M32), (seed & M32, (seed >> 32) & M32))
    u = (np.array(w, dtype=np.float64) + 0.5) * 2.0 ** -32
    out = np.empty(4)
    for h in (0, 2):
        r, a = np.sqrt(-2.0 * np.log(u[h])), 6.283185307179586 * u[h + 1]
        out[h], out[h + 1] = r * np.cos(a), r * np.sin(a)
    return out


def sense(state, sensor, seed, period, id_base=0):
    """state [B,>=4], sensor [B,8] -> est [B,4]"""
    state, sensor = np.asarray(state, dtype=np.float64), np.asarray(sensor, dtype=np.float64)
    B = len(state)
    est = state[:, 0:4] + sensor[:, 4:8]
    n = np.array([normals(seed, id_base + b, period) for b in range(B)]).reshape(B, 4)
    noisy = sensor[:, 0:4] != 0.0
    est = np.where(noisy, est + sensor[:, 0:4] * n, est)
    psi = est[:, 2]
    out_of_range = ~((psi >= -np.pi) & (psi < np.pi))
    est[:, 2] = np.where(out_of_range, (psi + np.pi) % (2.0 * np.pi) - np.pi, psi)
    est[:, 3] = np.maximum(0.0, est[:, 3])
    return est


def draw_states(rng, B, vx_range=None):
    """random plant states and commands as tests/test_closed_loop.py::test_sim_kernel_matches_oracle draws them (a tenth of the vehicles standing);
    vx_range=(lo, hi): every vehicle moving with vx uniform in it -> (state [B,8], cmd [B,2])"""
    s0 = np.zeros((B, 8))
    s0[:, 0:2] = rng.uniform(-500, 500, (B, 2))
    s0[:, 2] = rng.uniform(-np.pi, np.pi, B)
    s0[:, 3] = np.where(rng.random(B) < 0.1, 0.0, rng.uniform(0, 20, B)) if vx_range is None else rng.uniform(vx_range[0], vx_range[1], B)
    s0[:, 4] = rng.normal(0, 0.2, B) * (s0[:, 3] > 0)
    s0[:, 5] = rng.normal(0, 0.1, B) * (s0[:, 3] > 0)
    s0[:, 6] = rng.uniform(-1, 1, B)
    s0[:, 7] = rng.uniform(-0.5, 0.5, B)
    cmd = np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.5, 0.5, B)], 1)
    return s0, cmd


SPREAD_SEED, SPREAD_B = 23, 300


def spread_case(gentle=False):
    """the per-vehicle-rows case shared by the CPU and the GPU test: every parameter independently within +-30 % of its default, vx in [2, 20] m/s,
    the other states and the commands as draw_states draws them.  The last 10 vehicles share vehicle 0's state and command: vehicles 290 and 299 on
    the default row, vehicle 291 + w differing from it in word w alone (+20 %).
    gentle=True: the same with lateral velocity, yaw rate, tyre angle and steering command at a tenth, which keeps every slip-angle tangent within
    the kernel's polynomial range 1/8 for the whole period (the full draws leave it: 2 % of the vehicles start outside) -> (state, cmd, rows)"""
    rng = np.random.default_rng(SPREAD_SEED)
    B = SPREAD_B
    s0, cmd = draw_states(rng, B, vx_range=(2.0, 20.0))
    rows = DEFAULT_ROW * rng.uniform(0.7, 1.3, (B, 8))
    s0[0, 3:6] = (8.0, 0.15, 0.08)      # vehicle 0 is cornering: every word of the row acts on it within one period
    s0[0, 7], cmd[0] = 0.2, (0.7, -0.3)
    s0[B - 10:] = s0[0]
    cmd[B - 10:] = cmd[0]
    rows[B - 10:] = DEFAULT_ROW
    for w in range(8):
        rows[B - 9 + w, w] *= 1.2
    if gentle:
        s0[:, 4:6] *= 0.1
        s0[:, 7] *= 0.1
        cmd[:, 1] *= 0.1
    return s0, cmd, rows
