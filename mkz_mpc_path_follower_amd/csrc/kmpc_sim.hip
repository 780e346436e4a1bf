// kmpc_sim.hip -- batched vehicle simulator for closed-loop runs, gfx950 only.
// Restates scripts/vehicle_simulator.py:58-113 for B vehicles at once: one thread per vehicle (the model is a
// 6-state ODE + 2 actuator lags -- there is nothing to share between lanes), fp64 like the reference, state kept in
// registers across all sub-steps of a call, so a 0.1 s control period (10 model updates = 100 Euler sub-steps) costs one
// read and one write of 64 B per vehicle.  FP contraction is off so that every product/sum rounds as in the reference; sin / cos / atan2 are the device
// math library's or short polynomials on their small-argument ranges (both <= 1-2 ulp from numpy's), so parity with the numpy checker is to rounding,
// not bit-exact (tests/test_closed_loop.py states the tolerance).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kmpc.h"   // KMPC_PLANT_*, KMPC_SENSOR_*: the row layouts
#include "kmpc_dispatch.h"
#include "kmpc_stage.h"

#pragma clang fp contract(off)

// The 100 serial sub-steps of a control period are what this kernel's time is (one thread per vehicle): per sub-step two atan2, a sin / cos
// pair of the heading, cos of the tyre angle and an fmod.  In the states a path follower visits their arguments are small, so the common case
// takes a short polynomial (<= 1 ulp-level error, like libm's) and anything else the library call:
//   atan2(y, x), x > 0, |y / x| <= 1/8 (slip angles): odd Taylor series to t^19 (next term 8^-21 / 21 < 1e-20 relative);
//   cos(d), |d| <= 0.6 (tyre angle, actuator-lagged command within +-0.5): even series to d^18;
//   sin / cos(psi), psi wrapped to [-pi, pi): quadrant reduction + the Taylor polynomials on |r| <= pi/4;
//   the heading wrap only when psi + pi has left [0, 2 pi).
// Round 3: the sub-step is ONE straight-line block.  With one wave per SIMD (4096 vehicles = 64 waves) nothing hides the latency of the dependent fp64
// chains, so the five polynomial evaluations of a sub-step must overlap each other -- as separate `if (small argument) poly else library` branches each sat
// in its own basic block and the scheduler could not interleave them (79 us per control period).  Now every polynomial is evaluated unconditionally (with
// explicit fma: they are approximations, not reference operations -- the MODEL arithmetic below keeps contraction off and rounds like numpy), the two
// slip-angle quotients share one reciprocal, and a single wave-uniform test sends the wave through the library calls when ANY lane's argument is outside a
// polynomial's range (never, for states a path follower visits).
__device__ __forceinline__ double sim_rcp(double x)   // 1 / x to ~1 ulp (operands are speeds of 1e-6 ... 1e2 m/s)
{
    double y = __builtin_amdgcn_rcp(x);
    double e = fma(-x, y, 1.0);
    y = fma(y, e, y);
    e = fma(-x, y, 1.0);
    return fma(y, e, y);
}
__device__ __forceinline__ double sim_atan_poly(double t)   // |t| <= 1/8: odd Taylor series to t^19
{
    const double z = t * t;
    double p = -1.0 / 19.0;
    p = fma(p, z, 1.0 / 17.0); p = fma(p, z, -1.0 / 15.0); p = fma(p, z, 1.0 / 13.0); p = fma(p, z, -1.0 / 11.0); p = fma(p, z, 1.0 / 9.0);
    p = fma(p, z, -1.0 / 7.0); p = fma(p, z, 1.0 / 5.0); p = fma(p, z, -1.0 / 3.0);
    return fma(t, z * p, t);
}
__device__ __forceinline__ double sim_cos_poly(double z)   // z = d^2, |d| <= pi/4 (0.6 for the tyre angle): even series to d^18
{
    double p = -1.0 / 6402373705728000.0;
    p = fma(p, z, 1.0 / 20922789888000.0); p = fma(p, z, -1.0 / 87178291200.0); p = fma(p, z, 1.0 / 479001600.0); p = fma(p, z, -1.0 / 3628800.0);
    p = fma(p, z, 1.0 / 40320.0); p = fma(p, z, -1.0 / 720.0); p = fma(p, z, 1.0 / 24.0); p = fma(p, z, -0.5);
    return fma(z, p, 1.0);
}
__device__ __forceinline__ double sim_sin_poly(double r, double z)   // |r| <= pi/4: odd series to r^17
{
    double p = 1.0 / 355687428096000.0;
    p = fma(p, z, -1.0 / 1307674368000.0); p = fma(p, z, 1.0 / 6227020800.0); p = fma(p, z, -1.0 / 39916800.0); p = fma(p, z, 1.0 / 362880.0);
    p = fma(p, z, -1.0 / 5040.0); p = fma(p, z, 1.0 / 120.0); p = fma(p, z, -1.0 / 6.0);
    return fma(r * z, p, r);
}
// sin / cos of the heading (kept wrapped to [-pi, pi) by the model): Cody-Waite reduction by pi/2 in two pieces + the polynomials on |r| <= pi/4
__device__ __forceinline__ void sim_sincos_poly(double x, double *s, double *c)
{
    const double k = rint(x * 0.63661977236758134308);
    double r = fma(-k, 1.57079632679489655800e+00, x);
    r = fma(-k, 6.12323399573676603587e-17, r);
    const double z = r * r;
    const double sr = sim_sin_poly(r, z), cr = sim_cos_poly(z);
    const int q = (int)k & 3;
    const double ss = (q & 1) ? cr : sr, cc = (q & 1) ? sr : cr;
    *s = (q & 2) ? -ss : ss;
    *c = ((q + 1) & 2) ? -cc : cc;
}

// a road row's constants of a call (sim_substep<true> only): KMPC_ROAD_*; lim = mu x the static axle load
struct sim_road { double a_long, a_lat, df_offset, acc_gain, lim_f, lim_r; };

// the plant's state: X, Y, psi, vx, vy, wz and the two lagged actuators, as a row of `state` [B,8] holds it
struct sim_state { double X, Y, psi, vx, vy, wz, acc, df; };

// grip bookkeeping of a call (sim_substep<true> only)
struct sim_grip {
    int sat_f, sat_r;          // clipped sub-steps
    double peak_f, peak_r;     // largest |C_alpha alpha| [N]
};

// ONE Euler sub-step of 1 ms (vehicle_simulator.py:75-113) towards the targets (acc_des, df_des): the body of all four plant kernels.
// The state comes in BY VALUE and the new state goes out through `n` (the grip bookkeeping likewise, g -> gn), and each word of `n` is written where
// it is computed: a kernel's own state variables then never have their address taken, so they are promoted to registers before inlining exactly as
// when the body stood in the kernel, and the velocities are not sunk behind the wrap's branch.  With the state passed by reference the four kernels
// computed the same bits on another schedule, 1 - 3 % slower at one wave per SIMD (profiles/stage_refactor_ab.txt).
// ROAD adds what include/kmpc.h lists for kmpc_sim_advance_road, each in a statement of its own after the expression it extends: the tyre model
// reads dfe = df + DF_OFFSET, vx's derivative acce = ACC_GAIN * acc, each axle's force is clipped at its limit (stage::clip: inside the limit the
// force keeps its own bits, a NaN passes) and counted, and the two specific forces are added after the sums they join -- so a neutral row
// (inf, inf, 0, 0, 0, 1) leaves the state of sim_substep<false> bit for bit.  The polynomials' ranges are statements about the state, not about the
// parameters, so one wave-uniform test picks between them and the library for every plant.
template <bool ROAD>
__device__ __forceinline__ void sim_substep(const sim_state z, sim_state &n, double acc_des, double df_des, double lf, double lr, double inv_m,
                                            double inv_Iz, double C_alpha_f, double C_alpha_r, double k_acc, double k_df, const sim_road rd, const sim_grip g,
                                            sim_grip &gn)
{
    const double X = z.X, Y = z.Y, psi = z.psi, vx = z.vx, vy = z.vy, wz = z.wz, acc = z.acc, df = z.df;
    const double deltaT = 0.01 / 10.0;                              // dt_model / disc_steps, :24,:69
    const double pi = 3.141592653589793;
    const bool moving = fabs(vx) > 1e-6;                            // :75
    const double yf = vy + lf * wz, yr = vy - lf * wz;              // :76, :77 (lf where lr is expected -- as in the reference)
    const double rvx = sim_rcp(vx);
    const double tf = yf * rvx, tr = yr * rvx;
    double dfe = df, acce = acc;
    if constexpr (ROAD) {
        dfe = df + rd.df_offset;                                     // the tyre angle the tyre model reads
        acce = rd.acc_gain * acc;                                    // the acceleration that acts
    }
    // polynomial ranges: x > 0 and |y / x| <= 1/8 for the slip angles (a caller-written state may carry vx < 0: atan2's own quadrant logic),
    // |d_f| <= 0.6, |psi| <= 4
    const bool in_range = (!moving || (vx > 0.0 && fabs(tf) <= 0.125 && fabs(tr) <= 0.125)) && fabs(dfe) <= 0.6 && fabs(psi) <= 4.0;
    double af = sim_atan_poly(tf), ar = sim_atan_poly(tr), cd = sim_cos_poly(dfe * dfe), sp, cp;
    sim_sincos_poly(psi, &sp, &cp);
    if (__any(!in_range)) {   // wave-uniform: some lane is outside a polynomial's range -> the library calls (per lane, where needed)
        if (moving && !(vx > 0.0 && fabs(tf) <= 0.125 && fabs(tr) <= 0.125)) { af = atan2(yf, vx); ar = atan2(yr, vx); }
        if (!(fabs(dfe) <= 0.6)) cd = cos(dfe);
        if (!(fabs(psi) <= 4.0)) sincos(psi, &sp, &cp);
    }
    const double alpha_f = moving ? dfe - af : 0.0;                 // :76
    const double alpha_r = moving ? -ar : 0.0;                      // :77
    double Fyf = C_alpha_f * alpha_f, Fyr = C_alpha_r * alpha_r;    // :80-81: what the linear tyre asks for
    if constexpr (ROAD) {
        const double Ff = Fyf, Fr = Fyr;
        Fyf = stage::clip(Ff, rd.lim_f);
        Fyr = stage::clip(Fr, rd.lim_r);
        gn.sat_f = g.sat_f + ((Ff > rd.lim_f || Ff < -rd.lim_f) ? 1 : 0);
        gn.sat_r = g.sat_r + ((Fr > rd.lim_r || Fr < -rd.lim_r) ? 1 : 0);
        gn.peak_f = fabs(Ff) > g.peak_f ? fabs(Ff) : g.peak_f;
        gn.peak_r = fabs(Fr) > g.peak_r ? fabs(Fr) : g.peak_r;
    }
    // :84 reads `acc - 1/m*Fyf*np.sin(self.df) + self.wz*self.vy` with m = 1840 an int: the reference is Python 2 (print statements,
    // no `from __future__ import division`), so 1/m is INTEGER division = 0 and the lateral-force drag term vanishes (:88 uses 1.0/m)
    double vx_s = vx + deltaT * (acce + wz * vy);
    if constexpr (ROAD) vx_s = vx_s + deltaT * rd.a_long;
    const double vx_n = fmax(0.0, vx_s);
    const bool fwd = vx_n > 1e-6;                                   // :87
    double vy_c = vy + deltaT * (inv_m * (Fyf * cd + Fyr) - wz * vx);                    // :88
    if constexpr (ROAD) vy_c = vy_c + deltaT * rd.a_lat;
    const double wz_c = wz + deltaT * (inv_Iz * (lf * Fyf * cd - lr * Fyr));             // :89
    const double vy_n = fwd ? vy_c : 0.0, wz_n = fwd ? wz_c : 0.0;                         // :91-92
    const double psi_n = psi + deltaT * wz;                         // :94
    const double X_n = X + deltaT * (vx * cp - vy * sp);            // :95
    const double Y_n = Y + deltaT * (vx * sp + vy * cp);            // :96
    n.X = X_n; n.Y = Y_n;
    n.vx = vx_n; n.vy = vy_n; n.wz = wz_n;
    const double a = psi_n + pi, p2 = 2.0 * pi;                     // :101  python's float % : result has the divisor's sign
    double md = a;
    const bool wrap = !(a >= 0.0 && a < p2);                        // (a % p2 == a exactly while a is inside [0, p2))
    if (__any(wrap)) {
        if (wrap) {
            md = fmod(a, p2);
            if (md < 0.0) md += p2;
        }
    }
    n.psi = md - pi;
    n.acc = k_acc * (acc_des - acc) * deltaT + acc;                 // :112
    n.df = k_df * (df_des - df) * deltaT + df;                    // :113
}

// without a road row
__device__ __forceinline__ void sim_substep(const sim_state z, sim_state &n, double acc_des, double df_des, double lf, double lr, double inv_m,
                                            double inv_Iz, double C_alpha_f, double C_alpha_r, double k_acc, double k_df)
{
    sim_grip gn;
    sim_substep<false>(z, n, acc_des, df_des, lf, lr, inv_m, inv_Iz, C_alpha_f, C_alpha_r, k_acc, k_df, sim_road{}, sim_grip{}, gn);
}

// the reference's plant: its constants, one command per call, the 10 n_updates sub-steps in one loop
__global__ __launch_bounds__(256) void kmpc_sim_kernel(int B, double *__restrict__ state, const double *__restrict__ cmd, int n_updates)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    double *s = state + 8 * (size_t)i;
    double X = s[0], Y = s[1], psi = s[2], vx = s[3], vy = s[4], wz = s[5], acc = s[6], df = s[7];
    const double acc_des = cmd[2 * (size_t)i], df_des = cmd[2 * (size_t)i + 1];
    for (int it = 0; it < n_updates * 10; ++it) {   // vehicle_simulator.py:61-67, :112-113: the reference's constants (the two quotients are folded)
        sim_state n;
        sim_substep(sim_state{X, Y, psi, vx, vy, wz, acc, df}, n, acc_des, df_des, 1.152, 1.693, 1.0 / 1840.0, 1.0 / 3477.0, 4.0703e4, 6.4495e4, 5.0, 5.0);
        X = n.X; Y = n.Y; psi = n.psi; vx = n.vx; vy = n.vy; wz = n.wz; acc = n.acc; df = n.df;
    }
    s[0] = X; s[1] = Y; s[2] = psi; s[3] = vx; s[4] = vy; s[5] = wz; s[6] = acc; s[7] = df;
}

hipError_t kmpc_launch_sim(int B, double *state, const double *cmd, int n_updates, hipStream_t st)
{
    hipLaunchKernelGGL(kmpc_sim_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, state, cmd, n_updates);
    return hipGetLastError();
}

// A plant per vehicle (kmpc_sim_advance_plant): the eight constants come from the vehicle's row `plant` [B,8] (KMPC_PLANT_*) -- 64 B more read per
// vehicle and call; a row holding kmpc_plant_default's values gives kmpc_sim_kernel's results bit for bit.
// Command delay: the first d = clamp(cmd_delay[i], 0, n_updates) updates (10 sub-steps each) run towards cmd_held[i], the rest towards cmd[i]; the
// target is a select per update, so lanes with different delays stay in one loop.  cmd[i] is then written to cmd_held[i].
__global__ __launch_bounds__(256) void kmpc_sim_plant_kernel(int B, double *__restrict__ state, const double *__restrict__ cmd,
                                                             const double *__restrict__ plant, const int32_t *__restrict__ cmd_delay,
                                                             double *__restrict__ cmd_held, int n_updates)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const double *pr = plant + KMPC_PLANT_WORDS * (size_t)i;
    const double lf = pr[KMPC_PLANT_LF], lr = pr[KMPC_PLANT_LR], m = pr[KMPC_PLANT_M], Iz = pr[KMPC_PLANT_IZ];
    const double C_alpha_f = pr[KMPC_PLANT_C_ALPHA_F], C_alpha_r = pr[KMPC_PLANT_C_ALPHA_R];
    const double k_acc = pr[KMPC_PLANT_K_ACC], k_df = pr[KMPC_PLANT_K_DF];
    const double inv_m = 1.0 / m, inv_Iz = 1.0 / Iz;   // divided once (correctly rounded, as the compiler folds 1.0 / 1840.0), multiplied as the source does
    double *s = state + 8 * (size_t)i;
    double X = s[0], Y = s[1], psi = s[2], vx = s[3], vy = s[4], wz = s[5], acc = s[6], df = s[7];
    const double acc_new = cmd[2 * (size_t)i], df_new = cmd[2 * (size_t)i + 1];
    int d = 0;
    double acc_old = acc_new, df_old = df_new;
    if (cmd_delay) {
        d = min(max(cmd_delay[i], 0), n_updates);
        acc_old = cmd_held[2 * (size_t)i]; df_old = cmd_held[2 * (size_t)i + 1];
    }
    for (int up = 0; up < n_updates; ++up) {
        const double acc_des = up < d ? acc_old : acc_new, df_des = up < d ? df_old : df_new;   // the target changes between updates only
#pragma unroll 1
        for (int it = 0; it < 10; ++it) {
            sim_state n;
            sim_substep(sim_state{X, Y, psi, vx, vy, wz, acc, df}, n, acc_des, df_des, lf, lr, inv_m, inv_Iz, C_alpha_f, C_alpha_r, k_acc, k_df);
            X = n.X; Y = n.Y; psi = n.psi; vx = n.vx; vy = n.vy; wz = n.wz; acc = n.acc; df = n.df;
        }
    }
    s[0] = X; s[1] = Y; s[2] = psi; s[3] = vx; s[4] = vy; s[5] = wz; s[6] = acc; s[7] = df;
    if (cmd_held) { cmd_held[2 * (size_t)i] = acc_new; cmd_held[2 * (size_t)i + 1] = df_new; }
}

hipError_t kmpc_launch_sim_plant(int B, double *state, const double *cmd, const double *plant, const int32_t *cmd_delay, double *cmd_held,
                                 int n_updates, hipStream_t st)
{
    hipLaunchKernelGGL(kmpc_sim_plant_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, state, cmd, plant, cmd_delay, cmd_held, n_updates);
    return hipGetLastError();
}

// The measurement stage (kmpc_sense_batch): est = truth + bias + sigma * n on the four state_est channels the MPC reads, one thread per vehicle.
// The normals are a pure function of (seed, id_base + b, period) -- Philox4x32-10 keyed by the seed, counter = (vehicle id, period), Box-Muller
// on the four words (include/kmpc.h has the specification) -- so a vehicle's noise does not depend on B, on the launch geometry or on the shard
// that simulates it.  A channel with sigma == 0 skips the noise term: est = truth + bias bit for bit.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4])
{
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// what both measurement kernels do once the truth t = x, y, psi, vx is fetched and the four Philox words w are drawn: bias, noise, the plant's wrap
// (:101; a heading in range passes unchanged) and the steering report's speed floor
__device__ __forceinline__ void sim_measure(const double t[4], const double *__restrict__ sr, const uint32_t w[4], double *__restrict__ o)
{
    double e[4];
    for (int c = 0; c < 4; ++c) e[c] = t[c] + sr[KMPC_SENSOR_BIAS_X + c];
    for (int h = 0; h < 2; ++h) {
        const double sg0 = sr[KMPC_SENSOR_SIGMA_X + 2 * h], sg1 = sr[KMPC_SENSOR_SIGMA_X + 2 * h + 1];
        if (sg0 != 0.0 || sg1 != 0.0) {
            const double u0 = ((double)w[2 * h] + 0.5) * 0x1p-32, u1 = ((double)w[2 * h + 1] + 0.5) * 0x1p-32;
            const double r = sqrt(-2.0 * log(u0)), a = 6.283185307179586 * u1;
            if (sg0 != 0.0) e[2 * h] = e[2 * h] + sg0 * (r * cos(a));
            if (sg1 != 0.0) e[2 * h + 1] = e[2 * h + 1] + sg1 * (r * sin(a));
        }
    }
    e[2] = stage::wrap(e[2]);
    e[3] = fmax(0.0, e[3]);              // the steering report's speed is not negative
    o[0] = e[0]; o[1] = e[1]; o[2] = e[2]; o[3] = e[3];
}

__global__ __launch_bounds__(256) void kmpc_sense_kernel(int B, const double *__restrict__ state, const double *__restrict__ sensor, uint64_t seed,
                                                         uint64_t period, uint64_t id_base, double *__restrict__ est)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const uint64_t gid = id_base + (uint64_t)i;
    uint32_t w[4];
    philox4x32_10((uint32_t)gid, (uint32_t)(gid >> 32), (uint32_t)period, (uint32_t)(period >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), w);
    const double *st = state + 8 * (size_t)i;
    double t[4];
    for (int c = 0; c < 4; ++c) t[c] = st[c];
    sim_measure(t, sensor + KMPC_SENSOR_WORDS * (size_t)i, w, est + 4 * (size_t)i);
}

hipError_t kmpc_launch_sense(int B, const double *state, const double *sensor, uint64_t seed, uint64_t period, uint64_t id_base, double *est,
                             hipStream_t st)
{
    hipLaunchKernelGGL(kmpc_sense_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, state, sensor, seed, period, id_base, est);
    return hipGetLastError();
}

// The command stage of the node's loop for B vehicles (mpc_cmd_pub.jl): the waypoint helper's stop flag latches (:100-103); a latched vehicle
// is commanded accel -1.0 / steer 0.0 (:148-153) and keeps its rate-limit anchor, any other publishes the solver's first input -- whatever the
// solver status (:120-132, Q7) -- and remembers it as the anchor of the next solve (:140).
__global__ __launch_bounds__(256) void kmpc_command_kernel(int B, const double *__restrict__ u0, const int32_t *__restrict__ stop, uint8_t *__restrict__ latch,
                                                           double *__restrict__ u_prev, double *__restrict__ cmd)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const bool st = latch[i] != 0 || stop[i] != 0;
    latch[i] = st ? 1 : 0;
    const double a = u0[2 * (size_t)i], d = u0[2 * (size_t)i + 1];
    cmd[2 * (size_t)i] = st ? -1.0 : a;
    cmd[2 * (size_t)i + 1] = st ? 0.0 : d;
    if (!st) { u_prev[2 * (size_t)i] = a; u_prev[2 * (size_t)i + 1] = d; }
}

hipError_t kmpc_launch_command(int B, const double *u0, const int32_t *stop, uint8_t *latch, double *u_prev, double *cmd, hipStream_t st)
{
    hipLaunchKernelGGL(kmpc_command_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, u0, stop, latch, u_prev, cmd);
    return hipGetLastError();
}

// A command queue (kmpc_sim_advance_queue): the one held command replaced by a ring of the last `depth` periods' commands, cmd_queue [depth,B,2]
// (slot j mod depth holds period j; consecutive lanes read consecutive 16 B), so that a command may take effect several control periods late.
// With d = clamp(cmd_delay, 0, (depth - 1) n) = q n + r the update `up` of period p runs towards the command of period p - q - (up < r): only two
// commands are in play per call.  sim_ring_commands logs this period's command, fetches the two -- period p - q (the later) and p - q - 1 (the
// earlier, needed only when r > 0; with q == depth - 1, r is 0 and its slot is this period's); a period before the first commands (0, 0) -- and
// returns r.
__device__ __forceinline__ int sim_ring_commands(double *cmd_queue, int depth, int B, int i, long long period, int n_updates,
                                                 const int32_t *__restrict__ cmd_delay, double acc_now, double df_now, double *acc_new,
                                                 double *df_new, double *acc_old, double *df_old)
{
    const size_t slot_words = 2 * (size_t)B;
    {
        double *own = cmd_queue + (size_t)(period % depth) * slot_words + 2 * (size_t)i;
        own[0] = acc_now; own[1] = df_now;
    }
    int d = cmd_delay ? cmd_delay[i] : 0;
    const long long dmax = (long long)(depth - 1) * n_updates;   // n_updates >= 1 here (the host returns before a launch otherwise)
    d = d < 0 ? 0 : ((long long)d > dmax ? (int)dmax : d);
    const int q = d / n_updates, r = d % n_updates;
    *acc_new = acc_now; *df_new = df_now; *acc_old = 0.0; *df_old = 0.0;
    const long long jn = period - q, jo = jn - 1;
    if (q > 0) {
        *acc_new = 0.0; *df_new = 0.0;
        if (jn >= 0) {
            const double *e = cmd_queue + (size_t)(jn % depth) * slot_words + 2 * (size_t)i;
            *acc_new = e[0]; *df_new = e[1];
        }
    }
    if (r > 0 && jo >= 0) {
        const double *e = cmd_queue + (size_t)(jo % depth) * slot_words + 2 * (size_t)i;
        *acc_old = e[0]; *df_old = e[1];
    }
    return r;
}

__global__ __launch_bounds__(256) void kmpc_sim_queue_kernel(int B, double *__restrict__ state, const double *__restrict__ cmd,
                                                             const double *__restrict__ plant, const int32_t *__restrict__ cmd_delay,
                                                             double *cmd_queue, int depth, long long period, int n_updates)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const double *pr = plant + KMPC_PLANT_WORDS * (size_t)i;
    const double lf = pr[KMPC_PLANT_LF], lr = pr[KMPC_PLANT_LR], m = pr[KMPC_PLANT_M], Iz = pr[KMPC_PLANT_IZ];
    const double C_alpha_f = pr[KMPC_PLANT_C_ALPHA_F], C_alpha_r = pr[KMPC_PLANT_C_ALPHA_R];
    const double k_acc = pr[KMPC_PLANT_K_ACC], k_df = pr[KMPC_PLANT_K_DF];
    const double inv_m = 1.0 / m, inv_Iz = 1.0 / Iz;   // divided once (correctly rounded, as the compiler folds 1.0 / 1840.0), multiplied as the source does
    double *s = state + 8 * (size_t)i;
    double X = s[0], Y = s[1], psi = s[2], vx = s[3], vy = s[4], wz = s[5], acc = s[6], df = s[7];
    double acc_new, df_new, acc_old, df_old;
    const int r = sim_ring_commands(cmd_queue, depth, B, i, period, n_updates, cmd_delay, cmd[2 * (size_t)i], cmd[2 * (size_t)i + 1], &acc_new, &df_new,
                                    &acc_old, &df_old);
    for (int up = 0; up < n_updates; ++up) {
        const double acc_des = up < r ? acc_old : acc_new, df_des = up < r ? df_old : df_new;   // the target changes between updates only
#pragma unroll 1
        for (int it = 0; it < 10; ++it) {
            sim_state n;
            sim_substep(sim_state{X, Y, psi, vx, vy, wz, acc, df}, n, acc_des, df_des, lf, lr, inv_m, inv_Iz, C_alpha_f, C_alpha_r, k_acc, k_df);
            X = n.X; Y = n.Y; psi = n.psi; vx = n.vx; vy = n.vy; wz = n.wz; acc = n.acc; df = n.df;
        }
    }
    s[0] = X; s[1] = Y; s[2] = psi; s[3] = vx; s[4] = vy; s[5] = wz; s[6] = acc; s[7] = df;
}

hipError_t kmpc_launch_sim_queue(int B, double *state, const double *cmd, const double *plant, const int32_t *cmd_delay, double *cmd_queue, int depth,
                                 long long period, int n_updates, hipStream_t st)
{
    hipLaunchKernelGGL(kmpc_sim_queue_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, state, cmd, plant, cmd_delay, cmd_queue, depth, period,
                       n_updates);
    return hipGetLastError();
}

// Grip and road (kmpc_sim_advance_road): the queue kernel with a road row per vehicle, `road` [B,8] (KMPC_ROAD_*), kept in registers like the plant
// row -- 64 B more read per vehicle and call -- and sim_substep<true>.
// Grip bookkeeping: per axle the number of clipped sub-steps and the largest |C_alpha alpha| of the call stay in registers (4 VGPRs + 2 counters);
// the utilisation is that maximum divided by the limit ONCE after the loop (a correctly rounded division by one positive number is monotone: the
// quotient of the maximum is the maximum of the quotients, bit for bit), so the sub-step carries no division.  road_stat [B,4] is read and
// written once, after the loop, and only when given.
__global__ __launch_bounds__(256) void kmpc_sim_road_kernel(int B, double *__restrict__ state, const double *__restrict__ cmd,
                                                            const double *__restrict__ plant, const double *__restrict__ road,
                                                            const int32_t *__restrict__ cmd_delay, double *cmd_queue, int depth, long long period,
                                                            int n_updates, double *__restrict__ road_stat)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const double *pr = plant + KMPC_PLANT_WORDS * (size_t)i;
    const double lf = pr[KMPC_PLANT_LF], lr = pr[KMPC_PLANT_LR], m = pr[KMPC_PLANT_M], Iz = pr[KMPC_PLANT_IZ];
    const double C_alpha_f = pr[KMPC_PLANT_C_ALPHA_F], C_alpha_r = pr[KMPC_PLANT_C_ALPHA_R];
    const double k_acc = pr[KMPC_PLANT_K_ACC], k_df = pr[KMPC_PLANT_K_DF];
    const double inv_m = 1.0 / m, inv_Iz = 1.0 / Iz;   // divided once (correctly rounded, as the compiler folds 1.0 / 1840.0), multiplied as the source does
    const double *rr = road + KMPC_ROAD_WORDS * (size_t)i;
    const sim_road rd{rr[KMPC_ROAD_A_LONG], rr[KMPC_ROAD_A_LAT], rr[KMPC_ROAD_DF_OFFSET], rr[KMPC_ROAD_ACC_GAIN],
                      rr[KMPC_ROAD_MU_F] * (m * 9.81 * lr / (lf + lr)),    // mu x the static axle loads, divided once per call
                      rr[KMPC_ROAD_MU_R] * (m * 9.81 * lf / (lf + lr))};
    int sat_f = 0, sat_r = 0;           // clipped sub-steps of this call
    double peak_f = 0.0, peak_r = 0.0;  // largest |C_alpha alpha| of this call [N]
    double *s = state + 8 * (size_t)i;
    double X = s[0], Y = s[1], psi = s[2], vx = s[3], vy = s[4], wz = s[5], acc = s[6], df = s[7];
    double acc_new, df_new, acc_old, df_old;
    const int r = sim_ring_commands(cmd_queue, depth, B, i, period, n_updates, cmd_delay, cmd[2 * (size_t)i], cmd[2 * (size_t)i + 1], &acc_new, &df_new,
                                    &acc_old, &df_old);
    for (int up = 0; up < n_updates; ++up) {
        const double acc_des = up < r ? acc_old : acc_new, df_des = up < r ? df_old : df_new;   // the target changes between updates only
#pragma unroll 1
        for (int it = 0; it < 10; ++it) {
            sim_state n;
            sim_grip gn;
            sim_substep<true>(sim_state{X, Y, psi, vx, vy, wz, acc, df}, n, acc_des, df_des, lf, lr, inv_m, inv_Iz, C_alpha_f, C_alpha_r, k_acc, k_df, rd,
                              sim_grip{sat_f, sat_r, peak_f, peak_r}, gn);
            X = n.X; Y = n.Y; psi = n.psi; vx = n.vx; vy = n.vy; wz = n.wz; acc = n.acc; df = n.df;
            sat_f = gn.sat_f; sat_r = gn.sat_r; peak_f = gn.peak_f; peak_r = gn.peak_r;
        }
    }
    s[0] = X; s[1] = Y; s[2] = psi; s[3] = vx; s[4] = vy; s[5] = wz; s[6] = acc; s[7] = df;
    if (road_stat) {
        double *rs = road_stat + KMPC_ROAD_STAT_WORDS * (size_t)i;
        const double c_f = rs[KMPC_ROAD_STAT_SAT_F], c_r = rs[KMPC_ROAD_STAT_SAT_R], u_f = rs[KMPC_ROAD_STAT_UTIL_F], u_r = rs[KMPC_ROAD_STAT_UTIL_R];
        const double n_f = peak_f / rd.lim_f, n_r = peak_r / rd.lim_r;   // an infinite limit: 0 by the division itself
        rs[KMPC_ROAD_STAT_SAT_F] = c_f + (double)sat_f; rs[KMPC_ROAD_STAT_SAT_R] = c_r + (double)sat_r;
        rs[KMPC_ROAD_STAT_UTIL_F] = n_f > u_f ? n_f : u_f; rs[KMPC_ROAD_STAT_UTIL_R] = n_r > u_r ? n_r : u_r;
    }
}

hipError_t kmpc_launch_sim_road(int B, double *state, const double *cmd, const double *plant, const double *road, const int32_t *cmd_delay,
                                double *cmd_queue, int depth, long long period, int n_updates, double *road_stat, hipStream_t st)
{
    hipLaunchKernelGGL(kmpc_sim_road_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, state, cmd, plant, road, cmd_delay, cmd_queue, depth, period,
                       n_updates, road_stat);
    return hipGetLastError();
}

// Stale fixes (kmpc_sense_delayed_batch): kmpc_sense_kernel measuring the truth of period - L instead of this period's.  This period's x, y, psi, vx go
// into slot period mod depth of truth_ring [depth,B,4] (consecutive lanes write consecutive 32 B) and the measured truth comes out of slot
// (period - L) mod depth, L = clamp(meas_delay, 0, min(depth - 1, period)); bias and noise are this period's (counter = (vehicle id, period)): noise
// belongs to the moment of emission.
__global__ __launch_bounds__(256) void kmpc_sense_delayed_kernel(int B, const double *__restrict__ state, const double *__restrict__ sensor, uint64_t seed,
                                                                 uint64_t period, uint64_t id_base, const int32_t *__restrict__ meas_delay,
                                                                 double *truth_ring, int depth, double *__restrict__ est)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const uint64_t gid = id_base + (uint64_t)i;
    uint32_t w[4];
    philox4x32_10((uint32_t)gid, (uint32_t)(gid >> 32), (uint32_t)period, (uint32_t)(period >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), w);
    const double *st = state + 8 * (size_t)i;
    const size_t slot_words = 4 * (size_t)B;
    double t[4];
    for (int c = 0; c < 4; ++c) t[c] = st[c];
    {
        double *own = truth_ring + (size_t)(period % (uint64_t)depth) * slot_words + 4 * (size_t)i;
        for (int c = 0; c < 4; ++c) own[c] = t[c];
    }
    const uint64_t lmax = period < (uint64_t)(depth - 1) ? period : (uint64_t)(depth - 1);
    const int lraw = meas_delay[i];
    const uint64_t L = lraw <= 0 ? 0 : ((uint64_t)lraw > lmax ? lmax : (uint64_t)lraw);
    if (L > 0) {
        const double *old = truth_ring + (size_t)((period - L) % (uint64_t)depth) * slot_words + 4 * (size_t)i;
        for (int c = 0; c < 4; ++c) t[c] = old[c];
    }
    sim_measure(t, sensor + KMPC_SENSOR_WORDS * (size_t)i, w, est + 4 * (size_t)i);
}

hipError_t kmpc_launch_sense_delayed(int B, const double *state, const double *sensor, uint64_t seed, uint64_t period, uint64_t id_base,
                                     const int32_t *meas_delay, double *truth_ring, int depth, double *est, hipStream_t st)
{
    hipLaunchKernelGGL(kmpc_sense_delayed_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, state, sensor, seed, period, id_base, meas_delay,
                       truth_ring, depth, est);
    return hipGetLastError();
}
