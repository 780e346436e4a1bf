// kmpc_predict_dist.hip -- prediction ahead under estimated disturbances (kmpc_predict_ahead_dist_batch), gfx950 only.
// kmpc_latency.hip's predict-ahead on the OBSERVER's augmented model: the estimate is carried from the moment it was measured to the moment this
// period's command takes effect by Euler steps of 10 ms under the logged commands, and the three constant disturbances of kmpc_observe_batch's
// record act on every step: the vehicle travels along psi + dpsi + beta, steers by d_f + ddelta and accelerates by acc + da.  Without them an
// unmodelled steering offset of 0.05 rad turns the predicted heading by about 0.035 rad over 0.35 s of dead time.
// One thread per vehicle, fp64, nothing shared between lanes: no LDS, no cross-lane traffic.  Of the 320 B record eight words are read (0 ... 6 and
// 35: two 64 B sectors), the state lives in registers from the one read to the one write.  The Lm n + d steps of a vehicle are a serial chain of
// sin / cos (device library); tan / atan only when the command in force changes.  FP contraction is off so that every product / sum rounds as
// include/kmpc.h states it and tests/predict_dist_ref.py follows it.  A translation unit of its own: no existing kernel is built differently.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kmpc.h"   // KMPC_OBS_*: the record layout
#include "kmpc_dispatch.h"

#pragma clang fp contract(off)

namespace {

// floor(a / n) for n > 0, towards -infinity (C's division truncates towards 0)
__device__ __forceinline__ long long pd_floor_div(long long a, long long n) { return a >= 0 ? a / n : -((-a + n - 1) / n); }

__device__ __forceinline__ int pd_clamp(int v, int lo, long long hi) { return v < lo ? lo : ((long long)v > hi ? (int)hi : v); }

// the command of period j as the log has it: (0, 0) before the first period
__device__ __forceinline__ void pd_command(const double *__restrict__ hist, int depth, int B, int i, long long j, double *acc, double *d_f)
{
    *acc = 0.0; *d_f = 0.0;
    if (j >= 0) {
        const double *e = hist + ((size_t)(j % depth) * (size_t)B + (size_t)i) * 2;
        *acc = e[0]; *d_f = e[1];
    }
}

__device__ __forceinline__ double pd_wrap(double a)   // kmpc_observe_batch's wrap
{
    const double pi = 3.141592653589793, p2 = 2.0 * pi;
    if (!(a >= -pi && a < pi)) {
        double md = fmod(a + pi, p2);
        if (md < 0.0) md += p2;
        a = md - pi;
    }
    return a;
}

// kmpc_observe_batch's clip: compare-and-select, inside the cap a keeps its own bits
__device__ __forceinline__ double pd_clip(double a, double cap) { return a > cap ? cap : (a < -cap ? -cap : a); }

}   // namespace

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
    const int Lm = pd_clamp(meas_delay[i], 0, period < max_meas_delay ? period : (long long)max_meas_delay);
    const int d = pd_clamp(cmd_delay[i], 0, max_cmd_delay);
    const double h = 0.01;
    double x = rp[KMPC_OBS_X], y = rp[KMPC_OBS_Y], psi = rp[KMPC_OBS_PSI], v = rp[KMPC_OBS_V];
    const double dpsi = rp[KMPC_OBS_DPSI], ddelta = rp[KMPC_OBS_DDELTA], da = rp[KMPC_OBS_DA];
    const long long tau0 = (period - Lm) * n, tau1 = period * n + d;
    long long j_cur = 0;
    bool have = false;
    double acc = 0.0, beta = 0.0, sb = 0.0;
    for (long long tau = tau0; tau < tau1; ++tau) {
        const long long j = pd_floor_div(tau - d, n);
        if (!have || j != j_cur) {   // the command changes at most once per n steps: tan / atan stay off the per-step chain
            double d_f;
            pd_command(hist, depth, B, i, j, &acc, &d_f);
            const double de = d_f + ddelta;
            beta = atan(L_b / (L_a + L_b) * tan(de));
            sb = sin(beta);
            j_cur = j; have = true;
        }
        const double th = (psi + dpsi) + beta;
        const double s = sin(th), c = cos(th);
        const double xn = x + h * (v * c), yn = y + h * (v * s);
        const double pn = pd_wrap(psi + h * (v / L_b * sb));
        const double vn = v + h * (acc + da);
        x = xn; y = yn; psi = pn; v = vn < 0.0 ? 0.0 : vn;
    }
    o[0] = x; o[1] = y; o[2] = pd_wrap(psi + pd_clip(dpsi, psi_cap)); o[3] = v;
}

hipError_t kmpc_launch_predict_ahead_dist(int B, const double *rec, const double *est, const double *hist, int depth, long long period, int n,
                                          const int32_t *cmd_delay, const int32_t *meas_delay, int max_cmd_delay, int max_meas_delay, double L_a,
                                          double L_b, double psi_cap, double *z_out, hipStream_t st)
{
    hipLaunchKernelGGL(kmpc_predict_ahead_dist_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, rec, est, hist, depth, period, n, cmd_delay,
                       meas_delay, max_cmd_delay, max_meas_delay, L_a, L_b, psi_cap, z_out);
    return hipGetLastError();
}
