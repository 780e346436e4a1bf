// kmpc_latency.hip -- the controller's side of latency in the closed loops (kmpc_cmd_in_force_batch, kmpc_predict_ahead_batch), gfx950 only.
// The controller keeps a log of the commands it sent, cmd_hist [depth,B,2] (slot j mod depth holds period j's command; consecutive lanes read
// consecutive 16 B), and its own ASSUMED delays: cmd_delay [B] in model updates of 10 ms, meas_delay [B] in whole control periods.  From them
//   kmpc_cmd_in_force_batch   selects the command that acted on the vehicle over the period the estimator steps across (a pure selection), and
//   kmpc_predict_ahead_batch  carries the estimate from the moment it was measured to the moment this period's command takes effect, by Euler
//                             steps of 10 ms of the SOLVER's bicycle (kmpc_estimate_batch's PREDICT state equations, dt = 0.01 s) under the logged commands.
// One thread per vehicle, fp64, nothing shared between lanes: no LDS, no cross-lane traffic; z lives in registers from the one read to the one write.
// The Lm n + d steps of a vehicle are a serial chain of sin / cos (device library); tan / atan only when the command in force changes (at most
// Lm + d / n + 2 times).  FP contraction is off so that every product / sum rounds as include/kmpc.h states it and tests/latency_ref.py follows it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kmpc.h"
#include "kmpc_dispatch.h"

#pragma clang fp contract(off)

namespace {

// floor(a / n) for n > 0, towards -infinity (C's division truncates towards 0)
__device__ __forceinline__ long long lat_floor_div(long long a, long long n) { return a >= 0 ? a / n : -((-a + n - 1) / n); }

__device__ __forceinline__ int lat_clamp(int v, int lo, long long hi) { return v < lo ? lo : ((long long)v > hi ? (int)hi : v); }

// the command of period j as the log has it: (0, 0) before the first period (vehicle_simulator.py:21-22)
__device__ __forceinline__ void lat_command(const double *__restrict__ hist, int depth, int B, int i, long long j, double *acc, double *d_f)
{
    *acc = 0.0; *d_f = 0.0;
    if (j >= 0) {
        const double *e = hist + ((size_t)(j % depth) * (size_t)B + (size_t)i) * 2;
        *acc = e[0]; *d_f = e[1];
    }
}

__device__ __forceinline__ double lat_wrap(double a)   // kmpc_estimate_batch's wrap
{
    const double pi = 3.141592653589793, p2 = 2.0 * pi;
    if (!(a >= -pi && a < pi)) {
        double md = fmod(a + pi, p2);
        if (md < 0.0) md += p2;
        a = md - pi;
    }
    return a;
}

}   // namespace

__global__ __launch_bounds__(256) void kmpc_cmd_in_force_kernel(int B, const double *__restrict__ hist, int depth, long long period, int n,
                                                                const int32_t *__restrict__ cmd_delay, const int32_t *__restrict__ meas_delay,
                                                                int max_cmd_delay, int max_meas_delay, double *__restrict__ u_out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const int Lm = lat_clamp(meas_delay[i], 0, period < max_meas_delay ? period : (long long)max_meas_delay);
    const int d = lat_clamp(cmd_delay[i], 0, max_cmd_delay);
    const long long tau = (period - Lm - 1) * n + n / 2;       // the midpoint of the period the filter steps across
    double acc, d_f;
    lat_command(hist, depth, B, i, lat_floor_div(tau - d, n), &acc, &d_f);
    u_out[2 * (size_t)i] = acc; u_out[2 * (size_t)i + 1] = d_f;
}

__global__ __launch_bounds__(256) void kmpc_predict_ahead_kernel(int B, const double *z, const double *__restrict__ hist, int depth,
                                                                 long long period, int n, const int32_t *__restrict__ cmd_delay,
                                                                 const int32_t *__restrict__ meas_delay, int max_cmd_delay, int max_meas_delay,
                                                                 double L_a, double L_b, double *z_out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const int Lm = lat_clamp(meas_delay[i], 0, period < max_meas_delay ? period : (long long)max_meas_delay);
    const int d = lat_clamp(cmd_delay[i], 0, max_cmd_delay);
    const double h = 0.01;
    double x = z[4 * (size_t)i], y = z[4 * (size_t)i + 1], psi = z[4 * (size_t)i + 2], v = z[4 * (size_t)i + 3];
    const long long tau0 = (period - Lm) * n, tau1 = period * n + d;
    long long j_cur = 0;
    bool have = false;
    double acc = 0.0, beta = 0.0, sb = 0.0;
    for (long long tau = tau0; tau < tau1; ++tau) {
        const long long j = lat_floor_div(tau - d, n);
        if (!have || j != j_cur) {   // the command changes at most once per n steps: tan / atan stay off the per-step chain
            double d_f;
            lat_command(hist, depth, B, i, j, &acc, &d_f);
            beta = atan(L_b / (L_a + L_b) * tan(d_f));
            sb = sin(beta);
            j_cur = j; have = true;
        }
        const double ang = psi + beta;
        const double sa = sin(ang), ca = cos(ang);
        const double xn = x + h * (v * ca), yn = y + h * (v * sa);
        const double pn = lat_wrap(psi + h * (v / L_b * sb));
        const double vn = v + h * acc;
        x = xn; y = yn; psi = pn; v = vn < 0.0 ? 0.0 : vn;
    }
    double *o = z_out + 4 * (size_t)i;
    o[0] = x; o[1] = y; o[2] = psi; o[3] = v;
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
