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
#include "kmpc_plant_step.h"   // sim_substep, the row and state helpers, sim_plant_rows: shared with kmpc_drive.hip
#include "kmpc_measure.h"      // philox4x32_10, sim_delayed_truth, sim_measure: shared with kmpc_sense_faults.hip

#pragma clang fp contract(off)

// The five plant kernels are kmpc_sim_kernel here, three shells over kmpc_plant_step.h's one body sim_plant_rows<RING, ROAD>, and kmpc_sim_drive_kernel
// (kmpc_drive.hip), which keeps a loop of its own between the same prologue and epilogue helpers; kmpc_launch_plant starts all five.

// the reference's plant: its constants (vehicle_simulator.py:61-67, :112-113; the two quotients are folded), one command per call, the 10 n_updates
// sub-steps in one loop
__global__ __launch_bounds__(256) void kmpc_sim_kernel(int B, double *__restrict__ state, const double *__restrict__ cmd, int n_updates)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    double *s = state + 8 * (size_t)i;
    const sim_state z = load_state(s);
    double X = z.X, Y = z.Y, psi = z.psi, vx = z.vx, vy = z.vy, wz = z.wz, acc = z.acc, df = z.df;   // scalars of the kernel's own: see sim_substep
    const double acc_des = cmd[2 * (size_t)i], df_des = cmd[2 * (size_t)i + 1];
    for (int it = 0; it < n_updates * 10; ++it) {
        sim_state n;
        sim_substep(sim_state{X, Y, psi, vx, vy, wz, acc, df}, n, acc_des, df_des,
                    sim_plant{1.152, 1.693, 1840.0, 3477.0, 4.0703e4, 6.4495e4, 5.0, 5.0, 1.0 / 1840.0, 1.0 / 3477.0});
        X = n.X; Y = n.Y; psi = n.psi; vx = n.vx; vy = n.vy; wz = n.wz; acc = n.acc; df = n.df;
    }
    store_state(s, sim_state{X, Y, psi, vx, vy, wz, acc, df});
}

// A plant per vehicle (kmpc_sim_advance_plant): the eight constants come from the vehicle's row `plant` [B,8] (KMPC_PLANT_*) -- 64 B more read per
// vehicle and call; a row holding kmpc_plant_default's values gives kmpc_sim_kernel's results bit for bit.  With cmd_delay the first updates run
// towards cmd_held[i] (sim_held_commands); cmd[i] is then written to cmd_held[i].
__global__ __launch_bounds__(256) void kmpc_sim_plant_kernel(int B, double *__restrict__ state, const double *__restrict__ cmd,
                                                             const double *__restrict__ plant, const int32_t *__restrict__ cmd_delay,
                                                             double *__restrict__ cmd_held, int n_updates)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) sim_plant_rows<false, false>(B, i, state, cmd, plant, nullptr, cmd_delay, cmd_held, 0, 0, n_updates, nullptr);
}

// A command queue (kmpc_sim_advance_queue): the one held command replaced by a ring of the last `depth` periods' commands, cmd_queue [depth,B,2]
// (sim_ring_commands).
__global__ __launch_bounds__(256) void kmpc_sim_queue_kernel(int B, double *__restrict__ state, const double *__restrict__ cmd,
                                                             const double *__restrict__ plant, const int32_t *__restrict__ cmd_delay,
                                                             double *cmd_queue, int depth, long long period, int n_updates)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) sim_plant_rows<true, false>(B, i, state, cmd, plant, nullptr, cmd_delay, cmd_queue, depth, period, n_updates, nullptr);
}

// Grip and road (kmpc_sim_advance_road): the queue kernel with a road row per vehicle, `road` [B,8] (KMPC_ROAD_*), kept in registers like the plant
// row -- 64 B more read per vehicle and call -- sim_substep<true>, and the grip bookkeeping folded into road_stat [B,4] when given.
__global__ __launch_bounds__(256) void kmpc_sim_road_kernel(int B, double *__restrict__ state, const double *__restrict__ cmd,
                                                            const double *__restrict__ plant, const double *__restrict__ road,
                                                            const int32_t *__restrict__ cmd_delay, double *cmd_queue, int depth, long long period,
                                                            int n_updates, double *__restrict__ road_stat)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) sim_plant_rows<true, true>(B, i, state, cmd, plant, road, cmd_delay, cmd_queue, depth, period, n_updates, road_stat);
}

// the fifth plant kernel is kmpc_drive.hip's
__global__ void kmpc_sim_drive_kernel(int B, double *__restrict__ state, const double *__restrict__ cmd, const double *__restrict__ plant,
                                      const double *__restrict__ road, const double *__restrict__ drive, const double *__restrict__ llc_rows,
                                      double *__restrict__ llc_rec, const int32_t *__restrict__ cmd_delay, double *cmd_queue, int depth,
                                      long long period, int n_updates, double *__restrict__ road_stat);

hipError_t kmpc_launch_plant(kmpc_plant_kind kind, const PlantCall &k, hipStream_t st)
{
    const dim3 grid((k.B + 255) / 256), block(256);
    switch (kind) {
    case KMPC_PLANT_FIXED: return kmpc_launch(kmpc_sim_kernel, grid, block, 0, st, k.B, k.state, k.cmd, k.n_updates);
    case KMPC_PLANT_ROWS: return kmpc_launch(kmpc_sim_plant_kernel, grid, block, 0, st, k.B, k.state, k.cmd, k.plant, k.cmd_delay, k.cmd_log, k.n_updates);
    case KMPC_PLANT_QUEUE:
        return kmpc_launch(kmpc_sim_queue_kernel, grid, block, 0, st, k.B, k.state, k.cmd, k.plant, k.cmd_delay, k.cmd_log, k.depth, k.period, k.n_updates);
    case KMPC_PLANT_ROAD:
        return kmpc_launch(kmpc_sim_road_kernel, grid, block, 0, st, k.B, k.state, k.cmd, k.plant, k.road, k.cmd_delay, k.cmd_log, k.depth, k.period,
                           k.n_updates, k.road_stat);
    case KMPC_PLANT_DRIVE:
        return kmpc_launch(kmpc_sim_drive_kernel, grid, block, 0, st, k.B, k.state, k.cmd, k.plant, k.road, k.drive, k.llc_rows, k.llc_rec, k.cmd_delay,
                           k.cmd_log, k.depth, k.period, k.n_updates, k.road_stat);
    }
    return hipErrorInvalidValue;
}

// The measurement stage: est = truth + bias + sigma * n on the four state_est channels the MPC reads, one thread per vehicle.  The generator, the
// arithmetic from truth to estimate and the ring of truths -- philox4x32_10, sim_measure, sim_delayed_truth -- are kmpc_measure.h's:
// kmpc_sense_faults.hip shares them.  ONE body, vehicle i: the draw, this period's truth, with RING the truth of period - L in its place, the estimate.
template <bool RING>
__device__ __forceinline__ void sim_sense(int B, int i, const double *__restrict__ state, const double *__restrict__ sensor, uint64_t seed,
                                          uint64_t period, uint64_t id_base, const int32_t *__restrict__ meas_delay, double *truth_ring, int depth,
                                          double *__restrict__ est)
{
    const uint64_t gid = id_base + (uint64_t)i;
    uint32_t w[4];
    philox4x32_10((uint32_t)gid, (uint32_t)(gid >> 32), (uint32_t)period, (uint32_t)(period >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), w);
    const double *st = state + 8 * (size_t)i;
    double t[4];
    for (int c = 0; c < 4; ++c) t[c] = st[c];
    if constexpr (RING) sim_delayed_truth(t, truth_ring, depth, B, i, period, meas_delay);
    sim_measure(t, sensor + KMPC_SENSOR_WORDS * (size_t)i, w, est + 4 * (size_t)i);
}

// kmpc_sense_batch: this period's truth
__global__ __launch_bounds__(256) void kmpc_sense_kernel(int B, const double *__restrict__ state, const double *__restrict__ sensor, uint64_t seed,
                                                         uint64_t period, uint64_t id_base, double *__restrict__ est)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) sim_sense<false>(B, i, state, sensor, seed, period, id_base, nullptr, nullptr, 0, est);
}

// Stale fixes (kmpc_sense_delayed_batch): the truth of period - L, out of truth_ring [depth,B,4]; bias and noise are this period's (counter =
// (vehicle id, period)): noise belongs to the moment of emission.
__global__ __launch_bounds__(256) void kmpc_sense_delayed_kernel(int B, const double *__restrict__ state, const double *__restrict__ sensor, uint64_t seed,
                                                                 uint64_t period, uint64_t id_base, const int32_t *__restrict__ meas_delay,
                                                                 double *truth_ring, int depth, double *__restrict__ est)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) sim_sense<true>(B, i, state, sensor, seed, period, id_base, meas_delay, truth_ring, depth, est);
}

// meas_delay and truth_ring both NULL: this period's truth
hipError_t kmpc_launch_sense(int B, const double *state, const double *sensor, uint64_t seed, uint64_t period, uint64_t id_base,
                             const int32_t *meas_delay, double *truth_ring, int depth, double *est, hipStream_t st)
{
    const dim3 grid((B + 255) / 256), block(256);
    if (!meas_delay) return kmpc_launch(kmpc_sense_kernel, grid, block, 0, st, B, state, sensor, seed, period, id_base, est);
    return kmpc_launch(kmpc_sense_delayed_kernel, grid, block, 0, st, B, state, sensor, seed, period, id_base, meas_delay, truth_ring, depth, est);
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
