// kmpc_frenet_ref.hip -- batched Frenet reference from look-ahead waypoints on gfx950: the step between kmpc_waypoints_batch and
// kmpc_solve_batch_frenet.
//
// Replaces, for B vehicles at once, what the reference's Frenet node does with a received path before it solves
// (scripts/nodes_gazebo_sim/gazebo_sim_mpc_cmd_pub_frenet.jl): convert_msg_to_path_dict (:54-85: path in the vehicle frame, the origin put in
// front, cumulative chord length) followed by get_reference_frenet (scripts/sim_path_utils/nav_msgs_path_frenet.py:76-86):
//   fit_XY_s (:62-73)                 np.interp of x and y on the grid 0.5 i, i < ceil(s_end / 0.5) (np.arange), two cubic least-squares fits;
//   compute_curvature_poly (:44-59)   K = (x' y'' - y' x'') / (x'^2 + y'^2) of the two cubics on the grid 0.25 j, j < ceil(s_end / 0.25), and a cubic
//                                     least-squares fit of K, highest degree first;
//   psi_start (:84)                   atan2(Y'(0), X'(0)),
// and the node's update_init_cond(0, 0, -psi_start, v) (:128).
//
// One wavefront per vehicle, fp64.  The at most 58 path points live in LDS; the resampled values are never stored: lane l visits grid points
// l, l + 64, ... and keeps the seven power sums and the right-hand sides of the normal equations, on the scaled abscissa t = s / s_end (on s itself
// the 4 x 4 Gram matrix spans s_end^6 and loses the fit; on t its condition number is ~1e4), which are then summed over the wave.  The 4 x 4
// Cholesky factorisation and the substitutions are wave-uniform scalar work; the coefficients are mapped back to s by powers of 1 / s_end.
// The vehicle-frame transform, the chords and the SEQUENTIAL chord sum round as the Julia loop does (no FMA contraction), so that s_end and with
// it the two grid lengths are numpy's.
//
// Refusal (fit_status 1, k_poly = 0, psi_start = 0, z0 = (0, 0, 0, v)): fewer than four resample points (np.polyfit is rank-deficient there),
// any non-finite input or intermediate (v included: z0 then is 0), a Gram matrix that is not positive definite, or s_end > 8192 m -- which bounds
// the two loops at 256 + 512 trips per lane whatever a pose far from the path or a diverged plant hands in (the longest real window is
// 57 x 0.2 s x 20 m/s = 228 m).  Every output is always written and always finite.
#include "kmpc_common.h"
#include "kmpc_dispatch.h"
#include "kmpc_interp.h"   // np_interp

constexpr int FR_MAX_POINTS = 58;         // origin + 57 waypoints (horizon <= 56)
constexpr double FR_MAX_S_END = 8192.0;   // m

// running sums of a cubic least-squares fit on t: S[k] = sum t^k (k = 0..6) and the right-hand sides sum t^k f (k = 0..3) of NF functions
template <int NF> struct FrSums {
    double S[7], r[NF][4];
    DEV void clear()
    {
#pragma unroll
        for (int k = 0; k < 7; ++k) S[k] = 0.0;
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int k = 0; k < 4; ++k) r[f][k] = 0.0;
    }
    DEV void add(double t, const double (&v)[NF])
    {
        const double t2 = t * t, t3 = t2 * t;
        S[0] += 1.0; S[1] += t; S[2] += t2; S[3] += t3; S[4] += t2 * t2; S[5] += t2 * t3; S[6] += t3 * t3;
#pragma unroll
        for (int f = 0; f < NF; ++f) { r[f][0] += v[f]; r[f][1] += t * v[f]; r[f][2] += t2 * v[f]; r[f][3] += t3 * v[f]; }
    }
    DEV void reduce()   // wave-wide sums, uniform in every lane afterwards
    {
#pragma unroll
        for (int k = 0; k < 7; ++k) S[k] = dpp_sum(S[k]);
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int k = 0; k < 4; ++k) r[f][k] = dpp_sum(r[f][k]);
    }
    // normal equations G c = r with G[i][j] = S[i + j]: Cholesky G = L L^T, then c (ascending powers of t) in place of r.  false: G is not positive definite
    DEV bool solve()
    {
        double L[4][4];
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double d = S[2 * j];
#pragma unroll
            for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
            ok = ok && d > 0.0;
            const double p = sqrt(d);
            L[j][j] = p;
#pragma unroll
            for (int i = j + 1; i < 4; ++i) {
                double v = S[i + j];
#pragma unroll
                for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
                L[i][j] = v / p;
            }
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            double *c = r[f];
#pragma unroll
            for (int i = 0; i < 4; ++i) {   // L y = r
                double v = c[i];
#pragma unroll
                for (int k = 0; k < i; ++k) v -= L[i][k] * c[k];
                c[i] = v / L[i][i];
            }
#pragma unroll
            for (int i = 3; i >= 0; --i) {  // L^T c = y
                double v = c[i];
#pragma unroll
                for (int k = i + 1; k < 4; ++k) v -= L[k][i] * c[k];
                c[i] = v / L[i][i];
            }
        }
        return ok;
    }
};

__global__ __launch_bounds__(64) void kmpc_frenet_ref_kernel(FR f)
{
    __shared__ double px[FR_MAX_POINTS], py[FR_MAX_POINTS], ps[FR_MAX_POINTS];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= f.B) return;
    const int P = f.H + 2;   // the origin in front of the H + 1 waypoints (:56-59: zeros(1)); P <= 58 <= 64 lanes
    // ---- path in the vehicle frame (base_link), chords, cumulative chord length (:62-77) ------------------------------------------------------------
    const double X0 = f.pose[3 * (size_t)b], Y0 = f.pose[3 * (size_t)b + 1], yaw = f.pose[3 * (size_t)b + 2];
    double sn, cs;
    sincos(yaw, &sn, &cs);
    double xl = 0.0, yl = 0.0;
    if (lane >= 1 && lane < P) {
        const double *w = f.ref + ((size_t)b * (f.H + 1) + (lane - 1)) * 3;
        const double dx = __dsub_rn(w[0], X0), dy = __dsub_rn(w[1], Y0);
        xl = __dadd_rn(__dmul_rn(cs, dx), __dmul_rn(sn, dy));
        yl = __dsub_rn(__dmul_rn(cs, dy), __dmul_rn(sn, dx));
    }
    const double xp_ = __shfl_up(xl, 1), yp_ = __shfl_up(yl, 1);
    const double ex = __dsub_rn(xl, xp_), ey = __dsub_rn(yl, yp_);
    const double chord = __dsqrt_rn(__dadd_rn(__dmul_rn(ex, ex), __dmul_rn(ey, ey)));
    if (lane < P) { px[lane] = xl; py[lane] = yl; ps[lane] = chord; }
    WSYNC();
    double s_acc = 0.0, s_mine = 0.0;   // every lane runs the same sequential sum (LDS broadcast reads) and keeps its own prefix
    for (int k = 1; k < P; ++k) {
        s_acc = __dadd_rn(s_acc, ps[k]);
        if (k == lane) s_mine = s_acc;
    }
    WSYNC();
    if (lane < P) ps[lane] = s_mine;
    WSYNC();
    const double s_end = uniform_(s_acc);
    const double vb = f.v ? f.v[b] : 0.0;
    const bool v_ok = isfinite(vb);
    bool ok = !__any(!(isfinite(xl) && isfinite(yl))) && s_end <= FR_MAX_S_END && v_ok;   // (NaN s_end fails the comparison)
    const int n1 = ok ? (int)ceil(s_end * 2.0) : 0;    // len(np.arange(0, s_end, 0.5))
    ok = ok && n1 >= 4;
    const int n2 = ok ? (int)ceil(s_end * 4.0) : 0;    // len(np.arange(0, s_end, 0.25))
    // ---- fit_XY_s (:62-73) ----------------------------------------------------------------------------------------------------------------------------
    FrSums<2> xy;
    xy.clear();
    for (int i = lane; i < (ok ? n1 : 0); i += 64) {
        const double s = 0.5 * (double)i;
        const double v[2] = {np_interp(s, ps, px, P), np_interp(s, ps, py, P)};
        xy.add(s / s_end, v);
    }
    xy.reduce();
    ok = xy.solve() && ok;
    const double *cx = xy.r[0], *cy = xy.r[1];   // X(t), Y(t), ascending powers of t = s / s_end
    // ---- compute_curvature_poly (:44-59) on the grid of :79 -----------------------------------------------------------------------------------------
    FrSums<1> kk;
    kk.clear();
    for (int j = lane; j < (ok ? n2 : 0); j += 64) {
        const double t = 0.25 * (double)j / s_end;
        const double xt = cx[1] + t * (2.0 * cx[2] + 3.0 * cx[3] * t), xtt = 2.0 * cx[2] + 6.0 * cx[3] * t;   // d/dt = s_end d/ds
        const double yt = cy[1] + t * (2.0 * cy[2] + 3.0 * cy[3] * t), ytt = 2.0 * cy[2] + 6.0 * cy[3] * t;
        const double v[1] = {(xt * ytt - yt * xtt) / ((xt * xt + yt * yt) * s_end)};                          // x' y'' - y' x'' over x'^2 + y'^2, in s
        kk.add(t, v);
    }
    kk.reduce();
    ok = kk.solve() && ok;
    const double rl = 1.0 / s_end;
    const double *ck = kk.r[0];
    double kp[4] = {ck[3] * rl * rl * rl, ck[2] * rl * rl, ck[1] * rl, ck[0]};   // highest degree first, in s
    double psi = atan2(cy[1], cx[1]);                                            // :84 (the common factor 1 / s_end > 0 drops out)
    ok = ok && isfinite(kp[0]) && isfinite(kp[1]) && isfinite(kp[2]) && isfinite(kp[3]) && isfinite(psi);
    if (!ok) { kp[0] = kp[1] = kp[2] = kp[3] = 0.0; psi = 0.0; }
    if (lane == 0) {
        double *o = f.k_poly + 4 * (size_t)b;
        o[0] = kp[0]; o[1] = kp[1]; o[2] = kp[2]; o[3] = kp[3];
        f.psi[b] = psi;
        f.status[b] = ok ? 0 : 1;
        if (f.z0) {
            double *z = f.z0 + 4 * (size_t)b;
            z[0] = 0.0; z[1] = 0.0; z[2] = ok ? -psi : 0.0; z[3] = v_ok ? vb : 0.0;
        }
    }
}

hipError_t kmpc_launch_frenet_ref(const FR &f, hipStream_t st)
{
    hipLaunchKernelGGL(kmpc_frenet_ref_kernel, dim3(f.B), dim3(64), 0, st, f);
    return hipGetLastError();
}
