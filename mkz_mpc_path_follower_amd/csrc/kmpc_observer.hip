// kmpc_observer.hip -- disturbance observer and command offset (kmpc_observe_batch, kmpc_cmd_offset_batch), gfx950 only.
// kmpc_estimator.hip's filter on the solver's model augmented with three constant disturbances: a course offset dpsi, a steering offset ddelta and an
// acceleration offset da.  One thread per vehicle, fp64, no LDS and no cross-lane traffic; the 37 live record words, the 16 row words, z and u are
// read once and the 40 record words written once (320 B in, 320 B out per vehicle and call, + 128 B row, 32 B est, and dist / innov / flags when
// asked for).  FP contraction is off and every new term is appended after the estimator's, as include/kmpc.h states it, so that with p0 = q_d = 0 the
// first four states and the 4 x 4 block of P are kmpc_estimate_batch's numbers and a numpy restatement (tests/observer_ref.py) follows the rest to
// the last few ulp of the device library's tan / atan / sin / cos.
// Registers: xh (7) + the upper triangle of P (28) stay in VGPRs from the read to the write.  A = F P is formed ONE ROW AT A TIME: row i of A reads
// only words of P whose two indices are >= i, and the new row i of P is written from that row of A alone, so seven words of A are live at a time, not 28.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kmpc.h"   // KMPC_OBS_*, KMPC_OBSPAR_*, KMPC_EST_FLAG_*: record and row layouts
#include "kmpc_dispatch.h"
#include "kmpc_stage.h"   // wrap, clip, finite

#pragma clang fp contract(off)

namespace {

constexpr int NS = 7, NP = 28;   // states, words of the upper triangle

// index of P_ij in the row-major upper triangle, either order of i and j
__device__ __forceinline__ constexpr int tri(int i, int j) { return i <= j ? i * NS - (i * (i - 1)) / 2 + (j - i) : j * NS - (j * (j - 1)) / 2 + (i - j); }

// the entries F has beside the identity: rows x, y: psi, v, dpsi, ddelta; row psi: v, ddelta; row v: da
__device__ __forceinline__ constexpr bool has(int i, int k) { return i <= 1 ? (k >= 2 && k <= 5) : i == 2 ? (k == 3 || k == 5) : i == 3 ? k == 6 : false; }

}   // namespace

__global__ __launch_bounds__(256) void kmpc_observe_kernel(int B, double *__restrict__ rec, const double *z, const double *__restrict__ u,
                                                           int u_stride, const double *__restrict__ params, double dt, double L_a, double L_b,
                                                           double gate, double v_min, double psi_cap, double *est_out,
                                                           double *__restrict__ dist_out, double *__restrict__ innov_out,
                                                           int32_t *__restrict__ flags_out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    double *rp = rec + KMPC_OBS_WORDS * (size_t)i;
    const double *pp = params + KMPC_OBSPAR_WORDS * (size_t)i, *zp = z + 4 * (size_t)i, *up = u + (size_t)u_stride * (size_t)i;
    double xh[NS], P[NP], zz[4], q2[NS], r2[4], p02[3], nu_out[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < NS; ++a) {
        xh[a] = rp[KMPC_OBS_X + a];
        const double q = pp[KMPC_OBSPAR_Q_X + a];
        q2[a] = q * q;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        zz[c] = zp[c];
        const double r = pp[KMPC_OBSPAR_R_X + c];
        r2[c] = r * r;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double p0 = pp[KMPC_OBSPAR_P0_DPSI + a];
        p02[a] = p0 * p0;
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) P[k] = rp[KMPC_OBS_P + k];
    double count = rp[KMPC_OBS_COUNT], skipped = rp[KMPC_OBS_SKIPPED];
    const double acc = up[0], d_f = up[1];
    int flags = 0;
    bool fresh_out = false;   // the record leaves this call fresh (all zeros), est_out = z and dist_out = 0
    bool init = false;        // the record was initialised by this call: est_out = z bit for bit

    if (count == 0.0) {
        // first call on a fresh record: no predict; xh = (z, 0, 0, 0) and P = diag(r^2, p0^2) -- or, with a non-finite z, nothing at all
        bool ok = true;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (!stage::finite(zz[c])) { ok = false; flags |= 1 << c; }
        }
        if (ok) {
#pragma unroll
            for (int c = 0; c < 4; ++c) xh[c] = zz[c];
            xh[4] = 0.0; xh[5] = 0.0; xh[6] = 0.0;
#pragma unroll
            for (int k = 0; k < NP; ++k) P[k] = 0.0;
#pragma unroll
            for (int c = 0; c < 4; ++c) P[tri(c, c)] = r2[c];
#pragma unroll
            for (int a = 0; a < 3; ++a) P[tri(4 + a, 4 + a)] = p02[a];
            count = 1.0; skipped = 0.0;
            flags = KMPC_EST_FLAG_INIT;
            init = true;
        } else {
            fresh_out = true;
        }
    } else {
        // ---- predict: one Euler step of the solver's model under (acc + da, d_f + ddelta), travelling along psi + dpsi + beta
        const double de = d_f + xh[5];
        const double t = tan(de);
        const double k = L_b / (L_a + L_b);
        const double beta = atan(k * t);
        const double sb = sin(beta), cb = cos(beta);
        const double th = (xh[2] + xh[4]) + beta;
        const double s = sin(th), c = cos(th);
        const double bp = k * (1.0 + t * t) / (1.0 + (k * t) * (k * t));
        const double v = xh[3];
        double F[4][NS];   // only the entries has() names are ever read
        F[0][2] = -(dt * (v * s)); F[0][3] = dt * c; F[1][2] = dt * (v * c); F[1][3] = dt * s; F[2][3] = dt * (sb / L_b);
        F[0][4] = F[0][2]; F[1][4] = F[1][2]; F[0][5] = F[0][2] * bp; F[1][5] = F[1][2] * bp;
        F[2][5] = dt * (v / L_b * (cb * bp)); F[3][6] = dt;
        xh[0] = xh[0] + dt * (v * c);
        xh[1] = xh[1] + dt * (v * s);
        xh[2] = stage::wrap(xh[2] + dt * (v / L_b * sb));
        const double vn = v + dt * (acc + xh[6]);
        xh[3] = vn < 0.0 ? 0.0 : vn;
        // P <- F P F^T on the upper triangle, a row of A = F P at a time (header comment); sums left to right, the estimator's terms first
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            double A[NS];
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                A[j] = 0.0;
                if (j < a && (j < 2 || a == 3)) continue;   // never read below; its words of P already hold the new rows
                double acc_a = P[tri(a, j)];
#pragma unroll
                for (int m = 2; m < NS; ++m)
                    if (has(a, m)) acc_a = acc_a + F[a][m] * P[tri(m, j)];
                A[j] = acc_a;
            }
#pragma unroll
            for (int j = a; j < NS; ++j) {
                double pn = A[j];
                if (j < 4) {
#pragma unroll
                    for (int m = 2; m < NS; ++m)
                        if (has(j, m)) pn = pn + F[j][m] * A[m];
                }
                P[tri(a, j)] = pn;
            }
        }
        const bool frozen = v < v_min;   // dpsi and ddelta are not observable at rest: their random walk stops
#pragma unroll
        for (int a = 0; a < NS; ++a) {
            if ((a == 4 || a == 5) && frozen) continue;
            P[tri(a, a)] = P[tri(a, a)] + q2[a];
        }
        // ---- update: four scalar updates, x, y, psi, v, over seven states
        int nskip = 0;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            double nu = zz[ch] - xh[ch];
            if (ch == 2) nu = stage::wrap(nu);
            const double S = P[tri(ch, ch)] + r2[ch];
            const bool skip = !stage::finite(zz[ch]) || !(S > 0.0 && stage::finite(S)) || (gate > 0.0 && nu * nu > gate * gate * S);
            if (skip) {
                flags |= 1 << ch;
                ++nskip;
            } else {
                double col[NS], K[NS];
#pragma unroll
                for (int a = 0; a < NS; ++a) col[a] = P[tri(a, ch)];   // column ch of P before this channel's update
#pragma unroll
                for (int a = 0; a < NS; ++a) K[a] = col[a] / S;
#pragma unroll
                for (int a = 0; a < NS; ++a) xh[a] = xh[a] + K[a] * nu;
#pragma unroll
                for (int a = 0; a < NS; ++a)
#pragma unroll
                    for (int b = a; b < NS; ++b) P[tri(a, b)] = P[tri(a, b)] - K[a] * col[b];
                nu_out[ch] = nu / sqrt(S);
            }
        }
        xh[2] = stage::wrap(xh[2]);
        xh[3] = xh[3] < 0.0 ? 0.0 : xh[3];
        count = count + 1.0;
        skipped = skipped + (double)nskip;
        // ---- containment: a record with a non-finite word does not survive the call
        bool ok = stage::finite(count) && stage::finite(skipped);
#pragma unroll
        for (int a = 0; a < NS; ++a) ok = ok && stage::finite(xh[a]);
#pragma unroll
        for (int m = 0; m < NP; ++m) ok = ok && stage::finite(P[m]);
        if (!ok) {
            fresh_out = true;
            flags |= KMPC_EST_FLAG_RESET;
        }
    }
    if (fresh_out) {
#pragma unroll
        for (int a = 0; a < NS; ++a) xh[a] = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) nu_out[c] = 0.0;
#pragma unroll
        for (int m = 0; m < NP; ++m) P[m] = 0.0;
        count = 0.0; skipped = 0.0;
    }
#pragma unroll
    for (int a = 0; a < NS; ++a) rp[KMPC_OBS_X + a] = xh[a];
#pragma unroll
    for (int m = 0; m < NP; ++m) rp[KMPC_OBS_P + m] = P[m];
    rp[KMPC_OBS_COUNT] = count; rp[KMPC_OBS_SKIPPED] = skipped;
    rp[37] = 0.0; rp[38] = 0.0; rp[39] = 0.0;
    double *eo = est_out + 4 * (size_t)i;
    const double psi_out = stage::wrap(xh[2] + stage::clip(xh[4], psi_cap));
    const bool z_out = fresh_out || init;
    eo[0] = z_out ? zz[0] : xh[0];
    eo[1] = z_out ? zz[1] : xh[1];
    eo[2] = z_out ? zz[2] : psi_out;
    eo[3] = z_out ? zz[3] : xh[3];
    if (dist_out) {
        double *dp = dist_out + 3 * (size_t)i;
        dp[0] = xh[4]; dp[1] = xh[5]; dp[2] = xh[6];
    }
    if (innov_out) {
        double *io = innov_out + 4 * (size_t)i;
#pragma unroll
        for (int c = 0; c < 4; ++c) io[c] = nu_out[c];
    }
    if (flags_out) flags_out[i] = flags;
}

// between the command stage and the plant: the two input disturbances leave the command (include/kmpc.h: kmpc_cmd_offset_batch)
__global__ __launch_bounds__(256) void kmpc_cmd_offset_kernel(int B, const double *__restrict__ rec, const uint8_t *__restrict__ latch, double acc_cap,
                                                              double df_cap, double *__restrict__ cmd)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    if (latch && latch[i]) return;
    const double *rp = rec + KMPC_OBS_WORDS * (size_t)i;
    const double dd = rp[KMPC_OBS_DDELTA], da = rp[KMPC_OBS_DA], count = rp[KMPC_OBS_COUNT];
    if (count == 0.0 || !stage::finite(dd) || !stage::finite(da)) return;
    const double ca = stage::clip(da, acc_cap), cd = stage::clip(dd, df_cap);
    double *cp = cmd + 2 * (size_t)i;
    if (ca != 0.0) cp[0] = cp[0] - ca;
    if (cd != 0.0) cp[1] = cp[1] - cd;
}

hipError_t kmpc_launch_observe(int B, double *rec, const double *z, const double *u, int u_stride, const double *params, double dt, double L_a,
                               double L_b, double gate, double v_min, double psi_cap, double *est_out, double *dist_out, double *innov_out,
                               int32_t *flags_out, hipStream_t st)
{
    hipLaunchKernelGGL(kmpc_observe_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, rec, z, u, u_stride, params, dt, L_a, L_b, gate, v_min,
                       psi_cap, est_out, dist_out, innov_out, flags_out);
    return hipGetLastError();
}

hipError_t kmpc_launch_cmd_offset(int B, const double *rec, const uint8_t *latch, double acc_cap, double df_cap, double *cmd, hipStream_t st)
{
    hipLaunchKernelGGL(kmpc_cmd_offset_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, rec, latch, acc_cap, df_cap, cmd);
    return hipGetLastError();
}
