"""TEST INFRASTRUCTURE: numpy restatement of the Gauss-Markov stage (kmpc_wander_batch), written from the text of include/kmpc.h, not from the
kernel, on top of plant_ref.philox4x32_10; and the mixed 300-vehicle case the GPU tests share.

Rows are [B,24] float64 (S0 words 0 ... 7, A words 8 ... 15, Q words 16 ... 23), records [B,16] (X words 0 ... 7, COUNT word 8), sensor and road
rows [B,8], all in the header's word order.  Every operation below is one numpy fp64 operation: rounded once, nothing contracted.
"""
import numpy as np

import plant_ref as R

CHANNELS, WORDS, REC_WORDS = 8, 24, 16
S0, A, Q = 0, 8, 16                    # KMPC_WANDER_S0 / _A / _Q: first word of each group
X, COUNT = 0, 8                        # KMPC_WANDERREC_*
CH_X, CH_Y, CH_PSI, CH_V, CH_A_LONG, CH_A_LAT, CH_DF_OFFSET, CH_FREE = range(8)   # KMPC_WANDER_CH_*
ROAD_WORD = {CH_A_LONG: 2, CH_A_LAT: 3, CH_DF_OFFSET: 4}   # channel -> KMPC_ROAD_* word
NEUTRAL = np.zeros(WORDS)
DOMAIN = (0x40000000, 0xC0000000)      # what call j XORs into the counter's last word


def words(seed, gid, period, j):
    """the four Philox words of call j (0 or 1) in period `period`: gid a Python int -> four ints, or an array of vehicle ids -> four uint64 arrays
    (plant_ref.philox4x32_10 is written in operations that numpy's uint64 arrays carry out without overflow: 32 x 32-bit products, shifts, xors)"""
    M = R.M32
    assert 0 <= period < 2 ** 62
    c3 = ((period >> 32) & M) ^ DOMAIN[j]
    key = (seed & M, (seed >> 32) & M)
    if isinstance(gid, (int, np.integer)):
        return R.philox4x32_10((int(gid) & M, (int(gid) >> 32) & M, period & M, c3), key)
    g = np.asarray(gid, dtype=np.uint64)
    return R.philox4x32_10((g & np.uint64(M), g >> np.uint64(32), np.full(g.shape, period & M, np.uint64), np.full(g.shape, c3, np.uint64)), key)


def normals(seed, gid, period):
    """the eight normals in period `period`: call j gives channels 4j ... 4j+3, paired as kmpc_sense_batch pairs its four.  gid an int -> [8];
    an array [B] of vehicle ids -> [B,8]"""
    g = np.atleast_1d(np.asarray(gid, dtype=np.uint64))
    out = np.empty((len(g), CHANNELS))
    for j in (0, 1):
        u = (np.stack(words(seed, g, period, j), 1).astype(np.float64) + 0.5) * 2.0 ** -32
        for h in (0, 2):
            r, a = np.sqrt(-2.0 * np.log(u[:, h])), 6.283185307179586 * u[:, h + 1]
            out[:, 4 * j + h], out[:, 4 * j + h + 1] = r * np.cos(a), r * np.sin(a)
    return out if np.ndim(gid) else out[0]


def active(rows):
    """[B,8] bool: a channel is off when S0 == 0 and Q == 0 (a NaN compares false: active)"""
    rows = np.asarray(rows, dtype=np.float64)
    return ~((rows[:, S0:S0 + 8] == 0.0) & (rows[:, Q:Q + 8] == 0.0))


def step(rows, rec, seed, period, id_base=0, sensor_base=None, road_base=None):
    """one call -> dict(rec [B,16], x [B,8], on [B,8], fresh [B], sensor_out, road_out ([B,8], or None without the base))"""
    rows, rec = np.asarray(rows, dtype=np.float64), np.asarray(rec, dtype=np.float64)
    B = len(rec)
    on = active(rows)
    n = normals(seed, id_base + np.arange(B, dtype=np.uint64), period).reshape(B, CHANNELS)
    count = rec[:, COUNT]
    with np.errstate(all="ignore"):
        fresh = ~(np.isfinite(count) & (count >= 0.0)) | (count == 0.0)
        first = rows[:, S0:S0 + 8] * n
        carried, fed = rows[:, A:A + 8] * rec[:, X:X + 8], rows[:, Q:Q + 8] * n
        x = np.where(on, np.where(fresh[:, None], first, carried + fed), 0.0)
        new = rec.copy()
        new[:, X:X + 8] = x
        new[:, COUNT] = np.where(fresh, 1.0, count + 1.0)
        sensor_out = road_out = None
        if sensor_base is not None:
            sensor_out = np.array(sensor_base, dtype=np.float64, copy=True)
            sensor_out[:, 4:8] = np.where(on[:, 0:4], sensor_out[:, 4:8] + x[:, 0:4], sensor_out[:, 4:8])
        if road_base is not None:
            road_out = np.array(road_base, dtype=np.float64, copy=True)
            for c, w in ROAD_WORD.items():
                road_out[:, w] = np.where(on[:, c], road_out[:, w] + x[:, c], road_out[:, w])
    return dict(rec=new, x=x, on=on, fresh=fresh, sensor_out=sensor_out, road_out=road_out)


def run(rows, seed, periods, id_base=0, rec=None, sensor_base=None, road_base=None):
    """consecutive calls over `periods` (an iterable of period numbers) from `rec` (default: fresh) -> dict of per-call arrays x [K,B,8],
    count [K,B], sensor_out, road_out [K,B,8] (when the base is given) and the last record `rec`"""
    rows = np.asarray(rows, dtype=np.float64)
    rec = np.zeros((len(rows), REC_WORDS)) if rec is None else np.array(rec, dtype=np.float64, copy=True)
    log = dict(x=[], count=[], sensor_out=[], road_out=[])
    for p in periods:
        o = step(rows, rec, seed, p, id_base, sensor_base, road_base)
        rec = o["rec"]
        log["x"].append(o["x"]); log["count"].append(rec[:, COUNT].copy())
        log["sensor_out"].append(o["sensor_out"]); log["road_out"].append(o["road_out"])
    out = {k: np.array(v) for k, v in log.items() if v and v[0] is not None}
    out["rec"] = rec
    return out


def stationary_rows(B, s0, a):
    """[B,24]: the same stationary row in every vehicle, Q = S0 * sqrt(1 - A^2)"""
    s0, a = np.asarray(s0, dtype=np.float64), np.asarray(a, dtype=np.float64)
    return np.tile(np.concatenate([s0, a, s0 * np.sqrt(1.0 - a * a)]), (B, 1))


# ---------------------------------------------------------------- the mixed case of the GPU tests
CASE_SEED, CASE_B, CASE_PERIODS, CASE_NOISE_SEED = 57, 300, 16, 0x9E3779B97F4A7C15


def mixed_case():
    """300 vehicles; the kind of channel c of vehicle b is (b + 3 c) % 6:
      0 stationary (S0 0.05 ... 1, A 0.5 ... 0.99, Q = S0 sqrt(1 - A^2))    1 white (A = 0, Q = S0)    2 constant (A = 1, Q = 0)
      3 walk (S0 = 0, A = 1, Q 0.01 ... 0.2)    4 off (all 0)    5 off with a carry-over (S0 = Q = 0, A = 0.7: still off)
    Vehicles 120 ... 129 are off in every channel, vehicles 130 ... 139 in channels 0 ... 3 only (no first Philox call), 140 ... 149 in channels
    4 ... 7 only.  Sensor and road base rows are drawn too, ten of them with a -0.0 bias.
    -> dict(rows [300,24], kind [300,8], sensor [300,8], road [300,8], seed)"""
    rng = np.random.default_rng(CASE_SEED)
    B = CASE_B
    kind = (np.arange(B)[:, None] + 3 * np.arange(8)[None, :]) % 6
    kind[120:130] = 4
    kind[130:140, 0:4] = 4
    kind[140:150, 4:8] = 5
    s0, a, q = rng.uniform(0.05, 1.0, (B, 8)), rng.uniform(0.5, 0.99, (B, 8)), rng.uniform(0.01, 0.2, (B, 8))
    rows = np.zeros((B, WORDS))
    rows[:, S0:S0 + 8] = np.where(kind <= 2, s0, 0.0)
    rows[:, A:A + 8] = np.select([kind == 0, kind == 1, (kind == 2) | (kind == 3), kind == 5], [a, 0.0, 1.0, 0.7], 0.0)
    rows[:, Q:Q + 8] = np.select([kind == 0, kind == 1, kind == 3], [s0 * np.sqrt(1.0 - a * a), s0, q], 0.0)
    sensor = np.concatenate([rng.uniform(0.0, 0.3, (B, 4)), rng.normal(0, 0.2, (B, 4))], 1)
    sensor[50:60, 4:8] = -0.0
    road = np.tile([np.inf, np.inf, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0], (B, 1))
    road[:, 0:2] = rng.uniform(0.3, 1.2, (B, 2))
    road[:, 2:5] = rng.normal(0, 1, (B, 3)) * [0.5, 1.0, 0.01]
    road[:, 5] = rng.uniform(0.8, 1.2, B)
    road[:, 6:8] = rng.normal(0, 1, (B, 2))          # read by nobody: must come through bit for bit
    road[50:60, 2:5] = -0.0
    return dict(rows=rows, kind=kind, sensor=sensor, road=road, seed=CASE_NOISE_SEED)
