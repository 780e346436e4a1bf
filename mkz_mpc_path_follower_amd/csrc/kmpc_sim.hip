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
#include "kmpc_plant_step.h"   // sim_substep, its polynomials, sim_ring_commands: shared with kmpc_drive.hip
#include "kmpc_measure.h"      // philox4x32_10, sim_measure: shared with kmpc_sense_faults.hip

#pragma clang fp contract(off)

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
// The generator and the arithmetic from truth to estimate, philox4x32_10 and sim_measure, are kmpc_measure.h's: kmpc_sense_faults.hip shares them.
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

// A command queue (kmpc_sim_advance_queue): the one held command replaced by a ring of the last `depth` periods' commands, cmd_queue [depth,B,2];
// sim_ring_commands (kmpc_plant_step.h) logs this period's command and fetches the two that are in play.
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
