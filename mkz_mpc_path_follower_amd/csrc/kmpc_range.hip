// kmpc_range.hip -- the range sensor and leader tracker (kmpc_range_follow_batch), gfx950 only: behind kmpc_follow_fleet, per vehicle a measured gap
// and leader speed, a two-state Kalman track that coasts through dropouts, and include/kmpc_follow.h's law on what the track believes.
// include/kmpc_range.h states the arithmetic, step by step; this is that text.  One thread per vehicle, fp64; the vehicle's sensor row (11 of 16
// words), follow row (4 of 8), record (16) and truth are fetched whole before the Philox rounds, so the loads are in flight during them, and
// everything is stored in one pass at the end: about 0.4 KB moved per vehicle and call.  The generator is kmpc_measure.h's.  Every operation of
// the filter and the law is an _rn intrinsic: no product and sum share a rounding.  No lane reads another vehicle's words.  Plain C++: vector
// stores, no inline assembly, no LDS, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kmpc_follow.h"   // KMPC_FOLLOW_*: the follow row's layout
#include "../../include/kmpc_range.h"    // KMPC_RANGE_*, KMPC_RANGEREC_*
#include "kmpc_dispatch.h"
#include "kmpc_stage.h"                  // stage::finite
#include "kmpc_measure.h"                // philox4x32_10, box_muller

#pragma clang fp contract(off)

__global__ __launch_bounds__(256) void kmpc_range_follow_kernel(RG w)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= w.B) return;
    double *rec = w.rec + KMPC_RANGEREC_WORDS * (size_t)b;
    double rr[KMPC_RANGE_R_V + 1], r[KMPC_RANGEREC_WORDS];
#pragma unroll
    for (int k = 0; k < KMPC_RANGE_R_V + 1; ++k) rr[k] = w.range_rows[KMPC_RANGE_WORDS * (size_t)b + k];
#pragma unroll
    for (int k = 0; k < KMPC_RANGEREC_WORDS; ++k) r[k] = rec[k];
    const double *fr = w.follow_rows + KMPC_FOLLOW_WORDS * (size_t)b;
    const double d_min = fr[KMPC_FOLLOW_D_MIN], t_h = fr[KMPC_FOLLOW_T_HEADWAY], a_b = fr[KMPC_FOLLOW_A_BRAKE], k_gap = fr[KMPC_FOLLOW_K_GAP];
    const double gap = w.truth[2 * (size_t)b], v_j = w.truth[2 * (size_t)b + 1];
    const int L = w.leader[b];
    const double v_t = w.speed_true[(size_t)b * w.true_stride], v_k = w.speed_known[(size_t)b * w.known_stride];
    const double cap = w.v_cap[b], dt = w.dt;

    // 1: the draws
    const uint64_t gid = w.id_base + (uint64_t)b;
    uint32_t pw[4];
    philox4x32_10((uint32_t)gid, (uint32_t)(gid >> 32), (uint32_t)w.period, (uint32_t)(w.period >> 32) ^ 0x20000000u, (uint32_t)w.seed,
                  (uint32_t)(w.seed >> 32), pw);
    const double sigma_r = rr[KMPC_RANGE_SIGMA_R], sigma_v = rr[KMPC_RANGE_SIGMA_V], bias_r = rr[KMPC_RANGE_BIAS_R];
    double n0 = 0.0, n1 = 0.0;
    if (sigma_r != 0.0 || sigma_v != 0.0) box_muller(pw[0], pw[1], &n0, &n1);   // a pair nobody needs is skipped
    const double u = __dmul_rn(__dadd_rn((double)pw[2], 0.5), 0x1p-32);

    // 2: detection
    const bool known_ok = stage::finite(v_k);
    const bool valid = L >= 0 && stage::finite(gap) && stage::finite(v_j) && stage::finite(v_t) && known_ok;
    const bool inr = valid && gap <= rr[KMPC_RANGE_RANGE_MAX];
    const bool drop = inr && u < rr[KMPC_RANGE_P_DROP];
    const bool det = inr && !drop;

    // 3: the measurement
    double z_r = gap;
    z_r = bias_r != 0.0 ? __dadd_rn(z_r, bias_r) : z_r;
    z_r = sigma_r != 0.0 ? __dadd_rn(z_r, __dmul_rn(sigma_r, n0)) : z_r;
    const double e_v = __dsub_rn(v_k, v_t);
    double z_v = e_v != 0.0 ? __dadd_rn(v_j, e_v) : v_j;
    z_v = sigma_v != 0.0 ? __dadd_rn(z_v, __dmul_rn(sigma_v, n1)) : z_v;

    // 4: the track
    const double r_gap = rr[KMPC_RANGE_R_GAP], r_v = rr[KMPC_RANGE_R_V], Ld = (double)L;
    double g_hat = r[KMPC_RANGEREC_GAP_HAT], v_hat = r[KMPC_RANGEREC_V_HAT];
    double p00 = r[KMPC_RANGEREC_P00], p01 = r[KMPC_RANGEREC_P01], p11 = r[KMPC_RANGEREC_P11];
    double tid = r[KMPC_RANGEREC_TRACK_ID], coast = r[KMPC_RANGEREC_COAST];
    double n_new = r[KMPC_RANGEREC_N_NEW], n_lost = r[KMPC_RANGEREC_N_LOST];
    const bool fresh = det && tid != Ld;
    if (fresh) {
        g_hat = z_r; v_hat = z_v;
        p00 = r_gap; p01 = 0.0; p11 = r_v;
        coast = 0.0; tid = Ld;
        n_new = __dadd_rn(n_new, 1.0);
    } else if (tid >= 0.0) {
        g_hat = __dadd_rn(g_hat, __dmul_rn(dt, __dsub_rn(v_hat, v_k)));
        const double t = __dmul_rn(dt, p11);
        p00 = __dadd_rn(__dadd_rn(p00, __dmul_rn(dt, __dadd_rn(__dmul_rn(2.0, p01), t))), rr[KMPC_RANGE_Q_GAP]);
        p01 = __dadd_rn(p01, t);
        p11 = __dadd_rn(p11, rr[KMPC_RANGE_Q_V]);
        if (det) {
            if (rr[KMPC_RANGE_FILTER] == 0.0) {
                g_hat = z_r; v_hat = z_v;
            } else {
                {   // range
                    const double S = __dadd_rn(p00, r_gap), k0 = __ddiv_rn(p00, S), k1 = __ddiv_rn(p01, S), y = __dsub_rn(z_r, g_hat);
                    g_hat = __dadd_rn(g_hat, __dmul_rn(k0, y));
                    v_hat = __dadd_rn(v_hat, __dmul_rn(k1, y));
                    p11 = __dsub_rn(p11, __dmul_rn(k1, p01));
                    p01 = __dsub_rn(p01, __dmul_rn(k0, p01));
                    p00 = __dsub_rn(p00, __dmul_rn(k0, p00));
                }
                {   // speed
                    const double S = __dadd_rn(p11, r_v), k0 = __ddiv_rn(p01, S), k1 = __ddiv_rn(p11, S), y = __dsub_rn(z_v, v_hat);
                    g_hat = __dadd_rn(g_hat, __dmul_rn(k0, y));
                    v_hat = __dadd_rn(v_hat, __dmul_rn(k1, y));
                    p00 = __dsub_rn(p00, __dmul_rn(k0, p01));
                    p01 = __dsub_rn(p01, __dmul_rn(k1, p01));
                    p11 = __dsub_rn(p11, __dmul_rn(k1, p11));
                }
            }
            coast = 0.0;
        } else {
            coast = __dadd_rn(coast, 1.0);
            const bool lost = coast > rr[KMPC_RANGE_COAST_MAX] || tid != Ld || !known_ok;
            tid = lost ? -1.0 : tid;
            n_lost = lost ? __dadd_rn(n_lost, 1.0) : n_lost;
        }
    }

    // 5: the law on what the track believes; 6: the error against the truth
    const bool track = tid >= 0.0;
    double v_out = cap, n_bound = r[KMPC_RANGEREC_N_BOUND], sum_e2 = r[KMPC_RANGEREC_SUM_EGAP2], max_e = r[KMPC_RANGEREC_MAX_EGAP];
    if (track) {
        const double g = __dsub_rn(g_hat, d_min), gp = g > 0.0 ? g : 0.0;
        const double at = __dmul_rn(a_b, t_h);
        const double rad = __dadd_rn(__dadd_rn(__dmul_rn(at, at), __dmul_rn(v_hat, v_hat)), __dmul_rn(__dmul_rn(2.0, a_b), gp));
        const double v_safe = __dsub_rn(__dsqrt_rn(rad), at);
        const double v_gap = __dadd_rn(v_hat, __dmul_rn(k_gap, __dsub_rn(g, __dmul_rn(t_h, v_k))));
        double v_f = v_gap < v_safe ? v_gap : v_safe;
        v_f = v_f > 0.0 ? v_f : 0.0;
        const bool bound = v_f < cap;
        v_out = bound ? v_f : cap;
        n_bound = bound ? __dadd_rn(n_bound, 1.0) : n_bound;
        const double e = __dsub_rn(g_hat, gap), ae = fabs(e);
        const bool e_ok = stage::finite(e);
        sum_e2 = e_ok ? __dadd_rn(sum_e2, __dmul_rn(e, e)) : sum_e2;
        max_e = (e_ok && ae > max_e) ? ae : max_e;
    }

    // one pass of stores
    rec[KMPC_RANGEREC_GAP_HAT] = g_hat; rec[KMPC_RANGEREC_V_HAT] = v_hat;
    rec[KMPC_RANGEREC_P00] = p00; rec[KMPC_RANGEREC_P01] = p01; rec[KMPC_RANGEREC_P11] = p11;
    rec[KMPC_RANGEREC_TRACK_ID] = tid; rec[KMPC_RANGEREC_COAST] = coast;
    rec[KMPC_RANGEREC_N] = __dadd_rn(r[KMPC_RANGEREC_N], 1.0);
    rec[KMPC_RANGEREC_N_DETECT] = det ? __dadd_rn(r[KMPC_RANGEREC_N_DETECT], 1.0) : r[KMPC_RANGEREC_N_DETECT];
    rec[KMPC_RANGEREC_N_DROP] = drop ? __dadd_rn(r[KMPC_RANGEREC_N_DROP], 1.0) : r[KMPC_RANGEREC_N_DROP];
    rec[KMPC_RANGEREC_N_OUT] = (valid && !inr) ? __dadd_rn(r[KMPC_RANGEREC_N_OUT], 1.0) : r[KMPC_RANGEREC_N_OUT];
    rec[KMPC_RANGEREC_N_NEW] = n_new; rec[KMPC_RANGEREC_N_LOST] = n_lost; rec[KMPC_RANGEREC_N_BOUND] = n_bound;
    rec[KMPC_RANGEREC_SUM_EGAP2] = sum_e2; rec[KMPC_RANGEREC_MAX_EGAP] = max_e;
    w.v_cap_out[b] = v_out;
    if (w.meas_out) {
        double *m = w.meas_out + 4 * (size_t)b;
        m[0] = det ? z_r : NAN; m[1] = det ? z_v : NAN; m[2] = det ? 1.0 : 0.0; m[3] = coast;
    }
}

hipError_t kmpc_launch_range_follow(const RG &w, hipStream_t st)
{
    return kmpc_launch(kmpc_range_follow_kernel, dim3(((unsigned)w.B + 255u) / 256u), dim3(256), 0, st, w);
}
