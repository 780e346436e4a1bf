// kmpc_latency.hip -- the controller's side of latency in the closed loops (kmpc_cmd_in_force_batch, kmpc_predict_ahead_batch,
// kmpc_predict_ahead_dist_batch), gfx950 only.
// The controller keeps a log of the commands it sent, cmd_hist [depth,B,2] (slot j mod depth holds period j's command; consecutive lanes read
// consecutive 16 B), and its own ASSUMED delays: cmd_delay [B] in model updates of 10 ms, meas_delay [B] in whole control periods.  From them
//   kmpc_cmd_in_force_batch        selects the command that acted on the vehicle over the period the estimator steps across (a pure selection),
//   kmpc_predict_ahead_batch       carries the estimate from the moment it was measured to the moment this period's command takes effect, by Euler
//                                  steps of 10 ms of the SOLVER's bicycle (kmpc_estimate_batch's PREDICT state equations, dt = 0.01 s) under the logged
//                                  commands, and
//   kmpc_predict_ahead_dist_batch  does the same on the OBSERVER's augmented model, from kmpc_observe_batch's record: the three constant disturbances
//                                  act on every step -- the vehicle travels along psi + dpsi + beta, steers by d_f + ddelta and accelerates by
//                                  acc + da.  Without them an unmodelled steering offset of 0.05 rad turns the predicted heading by about 0.035 rad
//                                  over 0.35 s of dead time.  Of the 320 B record eight words are read (0 ... 6 and 35: two 64 B sectors).
// The two prediction kernels are written out one after the other on the same helpers (kmpc_stage.h).  As two instantiations of one templated loop the
// disturbed kernel computed the same bits 1 % slower at B = 4096 (profiles/stage_refactor_ab.txt), so the loop is not shared.
// One thread per vehicle, fp64, nothing shared between lanes: no LDS, no cross-lane traffic; the state lives in registers from the one read to the one
// write.  The Lm n + d steps of a vehicle are a serial chain of sin / cos (device library); tan / atan only when the command in force changes (at most
// Lm + d / n + 2 times).  FP contraction is off so that every product / sum rounds as include/kmpc.h states it and tests/latency_ref.py and
// tests/predict_dist_ref.py follow it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kmpc.h"   // KMPC_OBS_*: the observer's record layout
#include "kmpc_dispatch.h"
#include "kmpc_stage.h"   // wrap, clip, floor_div, clamp_delay, command

#pragma clang fp contract(off)

__global__ __launch_bounds__(256) void kmpc_cmd_in_force_kernel(int B, const double *__restrict__ hist, int depth, long long period, int n,
                                                                const int32_t *__restrict__ cmd_delay, const int32_t *__restrict__ meas_delay,
                                                                int max_cmd_delay, int max_meas_delay, double *__restrict__ u_out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const int Lm = stage::clamp_delay(meas_delay[i], 0, period < max_meas_delay ? period : (long long)max_meas_delay);
    const int d = stage::clamp_delay(cmd_delay[i], 0, max_cmd_delay);
    const long long tau = (period - Lm - 1) * n + n / 2;       // the midpoint of the period the filter steps across
    double acc, d_f;
    stage::command(hist, depth, B, i, stage::floor_div(tau - d, n), &acc, &d_f);
    u_out[2 * (size_t)i] = acc; u_out[2 * (size_t)i + 1] = d_f;
}

__global__ __launch_bounds__(256) void kmpc_predict_ahead_kernel(int B, const double *z, const double *__restrict__ hist, int depth,
                                                                 long long period, int n, const int32_t *__restrict__ cmd_delay,
                                                                 const int32_t *__restrict__ meas_delay, int max_cmd_delay, int max_meas_delay,
                                                                 double L_a, double L_b, double *z_out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const int Lm = stage::clamp_delay(meas_delay[i], 0, period < max_meas_delay ? period : (long long)max_meas_delay);
    const int d = stage::clamp_delay(cmd_delay[i], 0, max_cmd_delay);
    const double h = 0.01;
    double x = z[4 * (size_t)i], y = z[4 * (size_t)i + 1], psi = z[4 * (size_t)i + 2], v = z[4 * (size_t)i + 3];
    const long long tau0 = (period - Lm) * n, tau1 = period * n + d;
    long long j_cur = 0;
    bool have = false;
    double acc = 0.0, beta = 0.0, sb = 0.0;
    for (long long tau = tau0; tau < tau1; ++tau) {
        const long long j = stage::floor_div(tau - d, n);
        if (!have || j != j_cur) {   // the command changes at most once per n steps: tan / atan stay off the per-step chain
            double d_f;
            stage::command(hist, depth, B, i, j, &acc, &d_f);
            beta = atan(L_b / (L_a + L_b) * tan(d_f));
            sb = sin(beta);
            j_cur = j; have = true;
        }
        const double ang = psi + beta;
        const double sa = sin(ang), ca = cos(ang);
        const double xn = x + h * (v * ca), yn = y + h * (v * sa);
        const double pn = stage::wrap(psi + h * (v / L_b * sb));
        const double vn = v + h * acc;
        x = xn; y = yn; psi = pn; v = vn < 0.0 ? 0.0 : vn;
    }
    double *o = z_out + 4 * (size_t)i;
    o[0] = x; o[1] = y; o[2] = psi; o[3] = v;
}

__global__ __launch_bounds__(256) void kmpc_predict_ahead_dist_kernel(int B, const double *__restrict__ rec, const double *est,
                                                                      const double *__restrict__ hist, int depth, long long period, int n,
                                                                      const int32_t *__restrict__ cmd_delay, const int32_t *__restrict__ meas_delay,
                                                                      int max_cmd_delay, int max_meas_delay, double L_a, double L_b, double psi_cap,
                                                                      double *z_out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const double *rp = rec + KMPC_OBS_WORDS * (size_t)i, *ep = est + 4 * (size_t)i;
    double *o = z_out + 4 * (size_t)i;
    if (rp[KMPC_OBS_COUNT] == 0.0) {   // a fresh record has nothing to predict from: est comes back bit for bit
        const double e0 = ep[0], e1 = ep[1], e2 = ep[2], e3 = ep[3];
        o[0] = e0; o[1] = e1; o[2] = e2; o[3] = e3;
        return;
    }
    const int Lm = stage::clamp_delay(meas_delay[i], 0, period < max_meas_delay ? period : (long long)max_meas_delay);
    const int d = stage::clamp_delay(cmd_delay[i], 0, max_cmd_delay);
    const double h = 0.01;
    double x = rp[KMPC_OBS_X], y = rp[KMPC_OBS_Y], psi = rp[KMPC_OBS_PSI], v = rp[KMPC_OBS_V];
    const double dpsi = rp[KMPC_OBS_DPSI], ddelta = rp[KMPC_OBS_DDELTA], da = rp[KMPC_OBS_DA];
    const long long tau0 = (period - Lm) * n, tau1 = period * n + d;
    long long j_cur = 0;
    bool have = false;
    double acc = 0.0, beta = 0.0, sb = 0.0;
    for (long long tau = tau0; tau < tau1; ++tau) {
        const long long j = stage::floor_div(tau - d, n);
        if (!have || j != j_cur) {   // the command changes at most once per n steps: tan / atan stay off the per-step chain
            double d_f;
            stage::command(hist, depth, B, i, j, &acc, &d_f);
            const double de = d_f + ddelta;
            beta = atan(L_b / (L_a + L_b) * tan(de));
            sb = sin(beta);
            j_cur = j; have = true;
        }
        const double th = (psi + dpsi) + beta;
        const double s = sin(th), c = cos(th);
        const double xn = x + h * (v * c), yn = y + h * (v * s);
        const double pn = stage::wrap(psi + h * (v / L_b * sb));
        const double vn = v + h * (acc + da);
        x = xn; y = yn; psi = pn; v = vn < 0.0 ? 0.0 : vn;
    }
    o[0] = x; o[1] = y; o[2] = stage::wrap(psi + stage::clip(dpsi, psi_cap)); o[3] = v;
}

hipError_t kmpc_launch_cmd_in_force(int B, const double *hist, int depth, long long period, int n, const int32_t *cmd_delay, const int32_t *meas_delay,
                                    int max_cmd_delay, int max_meas_delay, double *u_out, hipStream_t st)
{
    hipLaunchKernelGGL(kmpc_cmd_in_force_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, hist, depth, period, n, cmd_delay, meas_delay,
                       max_cmd_delay, max_meas_delay, u_out);
    return hipGetLastError();
}

hipError_t kmpc_launch_predict_ahead(int B, const double *z, const double *hist, int depth, long long period, int n, const int32_t *cmd_delay,
                                     const int32_t *meas_delay, int max_cmd_delay, int max_meas_delay, double L_a, double L_b, double *z_out,
                                     hipStream_t st)
{
    hipLaunchKernelGGL(kmpc_predict_ahead_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, z, hist, depth, period, n, cmd_delay, meas_delay,
                       max_cmd_delay, max_meas_delay, L_a, L_b, z_out);
    return hipGetLastError();
}

hipError_t kmpc_launch_predict_ahead_dist(int B, const double *rec, const double *est, const double *hist, int depth, long long period, int n,
                                          const int32_t *cmd_delay, const int32_t *meas_delay, int max_cmd_delay, int max_meas_delay, double L_a,
                                          double L_b, double psi_cap, double *z_out, hipStream_t st)
{
    hipLaunchKernelGGL(kmpc_predict_ahead_dist_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, rec, est, hist, depth, period, n, cmd_delay,
                       meas_delay, max_cmd_delay, max_meas_delay, L_a, L_b, psi_cap, z_out);
    return hipGetLastError();
}
