// kmpc_plant_step.h -- what the plant kernels share (kmpc_sim.hip: the fixed plant and the three per-vehicle-row plants; kmpc_drive.hip: the
// pedal-driven plant): the Euler sub-step and its short polynomials, the row and state helpers around it, the two command sources, and the ONE body
// of the per-vehicle-row plants, sim_plant_rows.  A unit includes kmpc_stage.h before this header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kmpc.h"   // KMPC_PLANT_*, KMPC_ROAD_*, KMPC_ROAD_STAT_*: the row layouts

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

// a plant row's constants of a call: the eight words of KMPC_PLANT_* and the two reciprocals
struct sim_plant { double lf, lr, m, Iz, C_alpha_f, C_alpha_r, k_acc, k_df, inv_m, inv_Iz; };

__device__ __forceinline__ sim_plant load_plant(const double *__restrict__ row)
{
    const double m = row[KMPC_PLANT_M], Iz = row[KMPC_PLANT_IZ];
    return {row[KMPC_PLANT_LF], row[KMPC_PLANT_LR], m, Iz, row[KMPC_PLANT_C_ALPHA_F], row[KMPC_PLANT_C_ALPHA_R], row[KMPC_PLANT_K_ACC], row[KMPC_PLANT_K_DF],
            1.0 / m, 1.0 / Iz};   // divided once (correctly rounded, as the compiler folds 1.0 / 1840.0), multiplied as the source does
}

// a road row's constants of a call (sim_substep<true> only): KMPC_ROAD_*; lim = mu x the static axle load, divided once per call
struct sim_road { double a_long, a_lat, df_offset, acc_gain, lim_f, lim_r; };

__device__ __forceinline__ sim_road load_road(const double *__restrict__ row, const sim_plant &p)
{
    return {row[KMPC_ROAD_A_LONG], row[KMPC_ROAD_A_LAT], row[KMPC_ROAD_DF_OFFSET], row[KMPC_ROAD_ACC_GAIN],
            row[KMPC_ROAD_MU_F] * (p.m * 9.81 * p.lr / (p.lf + p.lr)), row[KMPC_ROAD_MU_R] * (p.m * 9.81 * p.lf / (p.lf + p.lr))};
}

// the plant's state: X, Y, psi, vx, vy, wz and the two lagged actuators, as a row of `state` [B,8] holds it
struct sim_state { double X, Y, psi, vx, vy, wz, acc, df; };

__device__ __forceinline__ sim_state load_state(const double *s) { return {s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]}; }
__device__ __forceinline__ void store_state(double *s, const sim_state z)
{
    s[0] = z.X; s[1] = z.Y; s[2] = z.psi; s[3] = z.vx; s[4] = z.vy; s[5] = z.wz; s[6] = z.acc; s[7] = z.df;
}

// grip bookkeeping of a call (sim_substep<true> only)
struct sim_grip {
    int sat_f, sat_r;          // clipped sub-steps
    double peak_f, peak_r;     // largest |C_alpha alpha| [N]
};

// Per axle the number of clipped sub-steps and the largest |C_alpha alpha| of the call stay in registers (4 VGPRs + 2 counters); the utilisation is
// that maximum divided by the limit ONCE after the loop (a correctly rounded division by one positive number is monotone: the quotient of the maximum
// is the maximum of the quotients, bit for bit), so the sub-step carries no division.  A vehicle's row of road_stat [B,4] is read and written once.
__device__ __forceinline__ void fold_road_stat(double *rs, const sim_grip &g, const sim_road &rd)
{
    const double c_f = rs[KMPC_ROAD_STAT_SAT_F], c_r = rs[KMPC_ROAD_STAT_SAT_R], u_f = rs[KMPC_ROAD_STAT_UTIL_F], u_r = rs[KMPC_ROAD_STAT_UTIL_R];
    const double n_f = g.peak_f / rd.lim_f, n_r = g.peak_r / rd.lim_r;   // an infinite limit: 0 by the division itself
    rs[KMPC_ROAD_STAT_SAT_F] = c_f + (double)g.sat_f; rs[KMPC_ROAD_STAT_SAT_R] = c_r + (double)g.sat_r;
    rs[KMPC_ROAD_STAT_UTIL_F] = n_f > u_f ? n_f : u_f; rs[KMPC_ROAD_STAT_UTIL_R] = n_r > u_r ? n_r : u_r;
}

// ONE Euler sub-step of 1 ms (vehicle_simulator.py:75-113) towards the targets (acc_des, df_des): the body of all five plant kernels.
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
__device__ __forceinline__ void sim_substep(const sim_state z, sim_state &n, double acc_des, double df_des, const sim_plant p, const sim_road rd,
                                            const sim_grip g, sim_grip &gn)
{
    const double X = z.X, Y = z.Y, psi = z.psi, vx = z.vx, vy = z.vy, wz = z.wz, acc = z.acc, df = z.df;
    const double lf = p.lf, lr = p.lr, inv_m = p.inv_m, inv_Iz = p.inv_Iz, C_alpha_f = p.C_alpha_f, C_alpha_r = p.C_alpha_r;
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
    n.acc = p.k_acc * (acc_des - acc) * deltaT + acc;                 // :112
    n.df = p.k_df * (df_des - df) * deltaT + df;                    // :113
}

// without a road row
__device__ __forceinline__ void sim_substep(const sim_state z, sim_state &n, double acc_des, double df_des, const sim_plant p)
{
    sim_grip gn;
    sim_substep<false>(z, n, acc_des, df_des, p, sim_road{}, sim_grip{}, gn);
}

// The two commands in play in a call: the update `up` runs towards the earlier one while up < r, towards the later one from then on.  The target
// is a select per update, so lanes with different delays stay in one loop.
struct sim_commands {
    double acc_new, df_new, acc_old, df_old;
    int r;
    __device__ __forceinline__ double acc(int up) const { return up < r ? acc_old : acc_new; }
    __device__ __forceinline__ double df(int up) const { return up < r ? df_old : df_new; }
};

// A held command (kmpc_sim_advance_plant): the first r = clamp(cmd_delay[i], 0, n_updates) updates run towards cmd_held[i], the rest towards this
// period's command; without cmd_delay every update runs towards this period's.
__device__ __forceinline__ sim_commands sim_held_commands(const double *cmd_held, int i, int n_updates, const int32_t *__restrict__ cmd_delay,
                                                          double acc_now, double df_now)
{
    sim_commands c{acc_now, df_now, acc_now, df_now, 0};
    if (cmd_delay) {
        c.r = min(max(cmd_delay[i], 0), n_updates);
        c.acc_old = cmd_held[2 * (size_t)i]; c.df_old = cmd_held[2 * (size_t)i + 1];
    }
    return c;
}

// A command queue (kmpc_sim_advance_queue): the one held command replaced by a ring of the last `depth` periods' commands, cmd_queue [depth,B,2]
// (slot j mod depth holds period j; consecutive lanes read consecutive 16 B), so that a command may take effect several control periods late.
// With d = clamp(cmd_delay, 0, (depth - 1) n) = q n + r the update `up` of period p runs towards the command of period p - q - (up < r): only two
// commands are in play per call.  sim_ring_commands logs this period's command and fetches the two -- period p - q (the later) and p - q - 1 (the
// earlier, needed only when r > 0; with q == depth - 1, r is 0 and its slot is this period's); a period before the first commands (0, 0).
__device__ __forceinline__ sim_commands sim_ring_commands(double *cmd_queue, int depth, int B, int i, long long period, int n_updates,
                                                          const int32_t *__restrict__ cmd_delay, double acc_now, double df_now)
{
    const size_t slot_words = 2 * (size_t)B;
    {
        double *own = cmd_queue + (size_t)(period % depth) * slot_words + 2 * (size_t)i;
        own[0] = acc_now; own[1] = df_now;
    }
    int d = cmd_delay ? cmd_delay[i] : 0;
    const long long dmax = (long long)(depth - 1) * n_updates;   // n_updates >= 1 here (the host returns before a launch otherwise)
    d = d < 0 ? 0 : ((long long)d > dmax ? (int)dmax : d);
    const int q = d / n_updates;
    sim_commands c{acc_now, df_now, 0.0, 0.0, d % n_updates};
    const long long jn = period - q, jo = jn - 1;
    if (q > 0) {
        c.acc_new = 0.0; c.df_new = 0.0;
        if (jn >= 0) {
            const double *e = cmd_queue + (size_t)(jn % depth) * slot_words + 2 * (size_t)i;
            c.acc_new = e[0]; c.df_new = e[1];
        }
    }
    if (c.r > 0 && jo >= 0) {
        const double *e = cmd_queue + (size_t)(jo % depth) * slot_words + 2 * (size_t)i;
        c.acc_old = e[0]; c.df_old = e[1];
    }
    return c;
}

// The ONE body of the per-vehicle-row plants (kmpc_sim_plant_kernel, kmpc_sim_queue_kernel, kmpc_sim_road_kernel are shells over it), vehicle i:
// the rows and the state into registers, the two commands in play from the command source -- RING: the ring cmd_log = cmd_queue [depth,B,2];
// otherwise the held command cmd_log = cmd_held [B,2] or null, which this period's command then replaces -- n_updates updates of 10 sub-steps,
// the state back, and with ROAD the vehicle's row of road_stat folded when given.  The state and the grip bookkeeping are scalars of the body's own
// that go into the sub-step as fresh structs by value and come out through fresh structs, so none has its address taken; kept in a struct of the
// body's across the loop they gave the same bits under another register assignment (profiles/plant_family_isa_diff.txt).
template <bool RING, bool ROAD>
__device__ __forceinline__ void sim_plant_rows(int B, int i, double *__restrict__ state, const double *__restrict__ cmd,
                                               const double *__restrict__ plant, const double *__restrict__ road,
                                               const int32_t *__restrict__ cmd_delay, double *cmd_log, int depth, long long period, int n_updates,
                                               double *__restrict__ road_stat)
{
    const sim_plant p = load_plant(plant + KMPC_PLANT_WORDS * (size_t)i);
    sim_road rd{};
    if constexpr (ROAD) rd = load_road(road + KMPC_ROAD_WORDS * (size_t)i, p);
    int sat_f = 0, sat_r = 0;           // clipped sub-steps of this call
    double peak_f = 0.0, peak_r = 0.0;  // largest |C_alpha alpha| of this call [N]
    double *s = state + 8 * (size_t)i;
    const sim_state z = load_state(s);
    double X = z.X, Y = z.Y, psi = z.psi, vx = z.vx, vy = z.vy, wz = z.wz, acc = z.acc, df = z.df;
    const double acc_now = cmd[2 * (size_t)i], df_now = cmd[2 * (size_t)i + 1];
    sim_commands c;
    if constexpr (RING) c = sim_ring_commands(cmd_log, depth, B, i, period, n_updates, cmd_delay, acc_now, df_now);
    else c = sim_held_commands(cmd_log, i, n_updates, cmd_delay, acc_now, df_now);
    for (int up = 0; up < n_updates; ++up) {
        const double acc_des = c.acc(up), df_des = c.df(up);   // the target changes between updates only
#pragma unroll 1
        for (int it = 0; it < 10; ++it) {
            sim_state n;
            sim_grip gn;
            sim_substep<ROAD>(sim_state{X, Y, psi, vx, vy, wz, acc, df}, n, acc_des, df_des, p, rd, sim_grip{sat_f, sat_r, peak_f, peak_r}, gn);
            X = n.X; Y = n.Y; psi = n.psi; vx = n.vx; vy = n.vy; wz = n.wz; acc = n.acc; df = n.df;
            if constexpr (ROAD) { sat_f = gn.sat_f; sat_r = gn.sat_r; peak_f = gn.peak_f; peak_r = gn.peak_r; }
        }
    }
    store_state(s, sim_state{X, Y, psi, vx, vy, wz, acc, df});
    if constexpr (!RING)
        if (cmd_log) { cmd_log[2 * (size_t)i] = acc_now; cmd_log[2 * (size_t)i + 1] = df_now; }
    if constexpr (ROAD)
        if (road_stat) fold_road_stat(road_stat + KMPC_ROAD_STAT_WORDS * (size_t)i, sim_grip{sat_f, sat_r, peak_f, peak_r}, rd);
}
