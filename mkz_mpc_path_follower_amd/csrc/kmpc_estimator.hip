// kmpc_estimator.hip -- batched state estimator between the measurement stage and the solver (kmpc_estimate_batch), gfx950 only.
// An extended Kalman filter on the SOLVER's model (MKZMPCPathFollower.jl's Euler bicycle with the handle's L_a, L_b), one thread per vehicle, fp64:
// the filter is a 4-state recursion with a 10-word covariance -- nothing to share between lanes, so no LDS and no cross-lane traffic.  The 16 record
// words, the 8 row words, z and u live in registers from the one read to the one write (128 B in, 128 B out per vehicle and call, + 32 B est, and
// innov / flags when asked for).  FP contraction is off so that every product / sum rounds as include/kmpc.h states it and a numpy restatement
// (tests/estimator_ref.py) follows it to the last few ulp of tan / atan / sin / cos, which are the device library's.
// H = I and R is diagonal: the measurement update is four scalar updates in the order x, y, psi, v (no matrix inverse); only the upper triangle of P
// is ever computed, so P stays symmetric by construction.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kmpc.h"   // KMPC_EST_*, KMPC_ESTPAR_*: record and row layouts
#include "kmpc_dispatch.h"
#include "kmpc_stage.h"   // wrap, finite

#pragma clang fp contract(off)

namespace {

// index of P_ij (i <= j) in the row-major upper triangle: xx xy xs xv | yy ys yv | ss sv | vv
__device__ __forceinline__ constexpr int tri(int i, int j) { return i * 4 - (i * (i - 1)) / 2 + (j - i); }

}   // namespace

__global__ __launch_bounds__(256) void kmpc_estimate_kernel(int B, double *__restrict__ rec, const double *z, const double *__restrict__ u,
                                                            int u_stride, const double *__restrict__ params, double dt, double L_a, double L_b,
                                                            double gate, double *est_out, double *__restrict__ innov_out,
                                                            int32_t *__restrict__ flags_out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    double *rp = rec + KMPC_EST_WORDS * (size_t)i;
    const double *pp = params + KMPC_ESTPAR_WORDS * (size_t)i, *zp = z + 4 * (size_t)i, *up = u + (size_t)u_stride * (size_t)i;
    double xh[4], P[10], zz[4], q2[4], r2[4], nu_out[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        xh[c] = rp[KMPC_EST_X + c];
        zz[c] = zp[c];
        const double q = pp[KMPC_ESTPAR_Q_X + c], r = pp[KMPC_ESTPAR_R_X + c];
        q2[c] = q * q; r2[c] = r * r;
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) P[k] = rp[KMPC_EST_PXX + k];
    double count = rp[KMPC_EST_COUNT], skipped = rp[KMPC_EST_SKIPPED];
    const double acc = up[0], d_f = up[1];
    int flags = 0;
    bool fresh_out = false;   // the record leaves this call fresh (all zeros) and est_out = z

    if (count == 0.0) {
        // first call on a fresh record: no predict; xh = z and P = diag(r^2) bit for bit -- or, with a non-finite z, nothing at all
        bool ok = true;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (!stage::finite(zz[c])) { ok = false; flags |= 1 << c; }
        }
        if (ok) {
#pragma unroll
            for (int c = 0; c < 4; ++c) xh[c] = zz[c];
#pragma unroll
            for (int k = 0; k < 10; ++k) P[k] = 0.0;
            P[tri(0, 0)] = r2[0]; P[tri(1, 1)] = r2[1]; P[tri(2, 2)] = r2[2]; P[tri(3, 3)] = r2[3];
            count = 1.0; skipped = 0.0;
            flags = KMPC_EST_FLAG_INIT;
        } else {
            fresh_out = true;
        }
    } else {
        // ---- predict: one Euler step of the solver's model, Jacobian at the state before the step
        const double beta = atan(L_b / (L_a + L_b) * tan(d_f));
        const double ang = xh[2] + beta;
        const double sa = sin(ang), ca = cos(ang), sb = sin(beta);
        const double v = xh[3];
        const double fxp = -(dt * (v * sa)), fxv = dt * ca, fyp = dt * (v * ca), fyv = dt * sa, fpv = dt * (sb / L_b);
        xh[0] = xh[0] + dt * (v * ca);
        xh[1] = xh[1] + dt * (v * sa);
        xh[2] = stage::wrap(xh[2] + dt * (v / L_b * sb));
        const double vn = v + dt * acc;
        xh[3] = vn < 0.0 ? 0.0 : vn;
        // A = F P (the entries the upper triangle of A F^T needs), then P <- A F^T + diag(q^2); sums left to right
        const double pxx = P[0], pxy = P[1], pxs = P[2], pxv = P[3], pyy = P[4], pys = P[5], pyv = P[6], pss = P[7], psv = P[8], pvv = P[9];
        const double Axx = pxx + fxp * pxs + fxv * pxv, Axy = pxy + fxp * pys + fxv * pyv;
        const double Axs = pxs + fxp * pss + fxv * psv, Axv = pxv + fxp * psv + fxv * pvv;
        const double Ayy = pyy + fyp * pys + fyv * pyv, Ays = pys + fyp * pss + fyv * psv, Ayv = pyv + fyp * psv + fyv * pvv;
        const double Ass = pss + fpv * psv, Asv = psv + fpv * pvv;
        P[0] = Axx + fxp * Axs + fxv * Axv + q2[0];
        P[1] = Axy + fyp * Axs + fyv * Axv;
        P[2] = Axs + fpv * Axv;
        P[3] = Axv;
        P[4] = Ayy + fyp * Ays + fyv * Ayv + q2[1];
        P[5] = Ays + fpv * Ayv;
        P[6] = Ayv;
        P[7] = Ass + fpv * Asv + q2[2];
        P[8] = Asv;
        P[9] = pvv + q2[3];
        // ---- update: four scalar updates, x, y, psi, v
        int nskip = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            double nu = zz[c] - xh[c];
            if (c == 2) nu = stage::wrap(nu);
            const double S = P[tri(c, c)] + r2[c];
            const bool skip = !stage::finite(zz[c]) || !(S > 0.0 && stage::finite(S)) || (gate > 0.0 && nu * nu > gate * gate * S);
            if (skip) {
                flags |= 1 << c;
                ++nskip;
            } else {
                double col[4], K[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) col[a] = a <= c ? P[tri(a, c)] : P[tri(c, a)];   // column c of P before this channel's update
#pragma unroll
                for (int a = 0; a < 4; ++a) K[a] = col[a] / S;
#pragma unroll
                for (int a = 0; a < 4; ++a) xh[a] = xh[a] + K[a] * nu;
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = a; b < 4; ++b) P[tri(a, b)] = P[tri(a, b)] - K[a] * col[b];
                nu_out[c] = nu / sqrt(S);
            }
        }
        xh[2] = stage::wrap(xh[2]);
        xh[3] = xh[3] < 0.0 ? 0.0 : xh[3];
        count = count + 1.0;
        skipped = skipped + (double)nskip;
        // ---- containment: a record with a non-finite word does not survive the call
        bool ok = stage::finite(count) && stage::finite(skipped);
#pragma unroll
        for (int c = 0; c < 4; ++c) ok = ok && stage::finite(xh[c]);
#pragma unroll
        for (int k = 0; k < 10; ++k) ok = ok && stage::finite(P[k]);
        if (!ok) {
            fresh_out = true;
            flags |= KMPC_EST_FLAG_RESET;
        }
    }
    if (fresh_out) {
#pragma unroll
        for (int c = 0; c < 4; ++c) { xh[c] = 0.0; nu_out[c] = 0.0; }
#pragma unroll
        for (int k = 0; k < 10; ++k) P[k] = 0.0;
        count = 0.0; skipped = 0.0;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) rp[KMPC_EST_X + c] = xh[c];
#pragma unroll
    for (int k = 0; k < 10; ++k) rp[KMPC_EST_PXX + k] = P[k];
    rp[KMPC_EST_COUNT] = count; rp[KMPC_EST_SKIPPED] = skipped;
    double *eo = est_out + 4 * (size_t)i;
#pragma unroll
    for (int c = 0; c < 4; ++c) eo[c] = fresh_out ? zz[c] : xh[c];
    if (innov_out) {
        double *io = innov_out + 4 * (size_t)i;
#pragma unroll
        for (int c = 0; c < 4; ++c) io[c] = nu_out[c];
    }
    if (flags_out) flags_out[i] = flags;
}

hipError_t kmpc_launch_estimate(int B, double *rec, const double *z, const double *u, int u_stride, const double *params, double dt, double L_a,
                                double L_b, double gate, double *est_out, double *innov_out, int32_t *flags_out, hipStream_t st)
{
    hipLaunchKernelGGL(kmpc_estimate_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, rec, z, u, u_stride, params, dt, L_a, L_b, gate, est_out,
                       innov_out, flags_out);
    return hipGetLastError();
}
