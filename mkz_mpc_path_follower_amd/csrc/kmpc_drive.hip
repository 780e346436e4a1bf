// kmpc_drive.hip -- the low-level controller as a stage (kmpc_llc_step_batch) and the pedal-driven plant (kmpc_sim_advance_drive), gfx950 only.
// The reference's test car never received MPC_cmd.accel_cmd as an acceleration: a 50 Hz node (src/LowLevelController.cpp) turned it into a throttle
// fraction, a brake torque and a steering-wheel angle.  kmpc_llc.h restates that node's control law as one device function; here it runs alone, one
// thread per controller, and inside the pedal-driven plant's loop, every second 10 ms update, in front of a powertrain that turns pedals into force.
// One thread per vehicle, the state, the record and all rows in registers across the call; no lane reads another's row.  include/kmpc.h states the
// arithmetic; contraction is off, every product and sum rounds on its own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kmpc.h"   // KMPC_PLANT_*, KMPC_ROAD_*, KMPC_DRIVE_*, KMPC_LLC_*, KMPC_LLCREC_*: the row layouts
#include "kmpc_dispatch.h"
#include "kmpc_stage.h"
#include "kmpc_plant_step.h"
#include "kmpc_llc.h"

#pragma clang fp contract(off)

// The stage alone: B controllers, one tick each.  speed: vehicle b's at speed[b * speed_stride] (sim.state + 3 with a stride of 8).
__global__ __launch_bounds__(256) void kmpc_llc_step_kernel(int B, const double *__restrict__ cmd, const double *__restrict__ speed, int speed_stride,
                                                            const double *__restrict__ par, double *__restrict__ rec, double *__restrict__ pedals_out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    double *r = rec + KMPC_LLCREC_WORDS * (size_t)i;
    llc::state s = llc::load(r);
    const llc::params p = llc::load_params(par + KMPC_LLC_WORDS * (size_t)i);
    llc::tick(s, p, speed[(size_t)i * (size_t)speed_stride], cmd[2 * (size_t)i], cmd[2 * (size_t)i + 1]);
    llc::store(r, s);   // the actuator words TH, BR are the plant's: not touched
    if (pedals_out) {
        double *o = pedals_out + 4 * (size_t)i;
        o[0] = s.th_cmd; o[1] = s.br_cmd; o[2] = s.wheel_cmd; o[3] = s.acc_cmd;
    }
}

hipError_t kmpc_launch_llc_step(int B, const double *cmd, const double *speed, int speed_stride, const double *llc_rows, double *llc_rec,
                                double *pedals_out, hipStream_t st)
{
    hipLaunchKernelGGL(kmpc_llc_step_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, cmd, speed, speed_stride, llc_rows, llc_rec, pedals_out);
    return hipGetLastError();
}

// The pedal-driven plant: the road plant with the controller's tick in front of every even absolute update and the powertrain after every sub-step.
// The tick, Fmax and the pedal lags interleave with the sub-step, so this kernel keeps a loop of its own instead of sim_plant_rows'; its prologue and
// epilogue are the same helpers (load_plant, load_road, load_state, sim_ring_commands, store_state, fold_road_stat: kmpc_plant_step.h).
// sim_substep<true> runs as it stands, with the tick's tyre-angle target; the acceleration lag it computes is overwritten (and removed by the
// compiler, K_ACC's load with it) by the net acceleration of the powertrain, which the NEXT sub-step's vx integrates exactly as it integrates `acc`
// in the other plants.  Per update: one division for the traction limit; per tick: one for the tyre-angle target; none inside the sub-step.
__global__ __launch_bounds__(256) void kmpc_sim_drive_kernel(int B, double *__restrict__ state, const double *__restrict__ cmd,
                                                             const double *__restrict__ plant, const double *__restrict__ road,
                                                             const double *__restrict__ drive, const double *__restrict__ llc_rows,
                                                             double *__restrict__ llc_rec, const int32_t *__restrict__ cmd_delay, double *cmd_queue,
                                                             int depth, long long period, int n_updates, double *__restrict__ road_stat)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const sim_plant p = load_plant(plant + KMPC_PLANT_WORDS * (size_t)i);
    const sim_road rd = load_road(road + KMPC_ROAD_WORDS * (size_t)i, p);
    const double *dr = drive + KMPC_DRIVE_WORDS * (size_t)i;
    const double F_peak = dr[KMPC_DRIVE_F_PEAK], P_max = dr[KMPC_DRIVE_P_MAX], k_th = dr[KMPC_DRIVE_K_TH], k_br = dr[KMPC_DRIVE_K_BR];
    const double c_roll = dr[KMPC_DRIVE_C_ROLL], c_drag = dr[KMPC_DRIVE_C_DRAG], ratio = dr[KMPC_DRIVE_STEER_RATIO];
    const double inv_r = 1.0 / dr[KMPC_DRIVE_WHEEL_RADIUS];   // divided once per call
    const llc::params lp = llc::load_params(llc_rows + KMPC_LLC_WORDS * (size_t)i);
    double *lrec = llc_rec + KMPC_LLCREC_WORDS * (size_t)i;
    llc::state ls = llc::load(lrec);
    double TH = lrec[KMPC_LLCREC_TH], BR = lrec[KMPC_LLCREC_BR];
    int sat_f = 0, sat_r = 0;           // clipped sub-steps of this call
    double peak_f = 0.0, peak_r = 0.0;  // largest |C_alpha alpha| of this call [N]
    double *s = state + 8 * (size_t)i;
    const sim_state z = load_state(s);
    double X = z.X, Y = z.Y, psi = z.psi, vx = z.vx, vy = z.vy, wz = z.wz, acc = z.acc, df = z.df;   // scalars of the kernel's own: see sim_substep
    const sim_commands c = sim_ring_commands(cmd_queue, depth, B, i, period, n_updates, cmd_delay, cmd[2 * (size_t)i], cmd[2 * (size_t)i + 1]);
    const double deltaT = 0.01 / 10.0;
    long long tau = period * (long long)n_updates;          // the absolute update
    double df_eff = ls.wheel_cmd / ratio;                    // the target held since the last tick (a fresh record: 0)
    for (int up = 0; up < n_updates; ++up, ++tau) {
        if ((tau & 1) == 0) {   // 50 Hz against the 100 Hz updates: the command in force for this update, the speed as it is now
            llc::tick(ls, lp, vx, c.acc(up), c.df(up));
            df_eff = ls.wheel_cmd / ratio;                   // the PLANT's true ratio: a ratio error is a steering gain error
        }
        const double vm = vx > 1.0 ? vx : 1.0;               // compare-and-select throughout: a NaN word poisons its own vehicle
        const double pw = P_max / vm;
        const double Fmax = pw < F_peak ? pw : F_peak;       // min(F_PEAK, P_MAX / max(vx, 1)): once per update
#pragma unroll 1
        for (int it = 0; it < 10; ++it) {
            sim_state n;
            sim_grip gn;
            sim_substep<true>(sim_state{X, Y, psi, vx, vy, wz, acc, df}, n, 0.0, df_eff, p, rd, sim_grip{sat_f, sat_r, peak_f, peak_r}, gn);
            TH = k_th * (ls.th_cmd - TH) * deltaT + TH;      // the pedal actuators lag
            BR = k_br * (ls.br_cmd - BR) * deltaT + BR;
            const double resist = n.vx > 1e-6 ? c_roll + c_drag * n.vx * n.vx : 0.0;   // rolling and air resistance, only while moving
            X = n.X; Y = n.Y; psi = n.psi; vx = n.vx; vy = n.vy; wz = n.wz; df = n.df;
            acc = p.inv_m * (TH * Fmax - BR * inv_r) - resist;  // state word 6: the powertrain's net longitudinal acceleration
            sat_f = gn.sat_f; sat_r = gn.sat_r; peak_f = gn.peak_f; peak_r = gn.peak_r;
        }
    }
    store_state(s, sim_state{X, Y, psi, vx, vy, wz, acc, df});
    llc::store(lrec, ls);
    lrec[KMPC_LLCREC_TH] = TH; lrec[KMPC_LLCREC_BR] = BR;
    if (road_stat) fold_road_stat(road_stat + KMPC_ROAD_STAT_WORDS * (size_t)i, sim_grip{sat_f, sat_r, peak_f, peak_r}, rd);
}
