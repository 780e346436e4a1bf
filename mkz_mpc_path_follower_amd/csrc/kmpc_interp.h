// kmpc_interp.h -- numpy's np.interp for one query point, shared by the waypoint kernel (kmpc_waypoints.hip) and the Frenet reference fit
// (kmpc_frenet_ref.hip).  No FMA contraction in slope * (x - xp[j]) + fp[j]: indices match numpy's bit for bit and values to the last ulp.
#pragma once
#include "kmpc_common.h"

// np.interp (numpy/core/src/multiarray/compiled_base.c arr_interp) for one query point
DEV double np_interp(double xq, const double *xp, const double *fp, int M)
{
    if (xq > xp[M - 1]) return fp[M - 1];
    if (xq < xp[0]) return fp[0];
    int lo = 0, hi = M;  // largest j with xp[j] <= xq
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (xp[mid] <= xq) lo = mid; else hi = mid; }
    const int j = lo;
    if (j == M - 1 || xp[j] == xq) return fp[j];
    const double slope = __ddiv_rn(__dsub_rn(fp[j + 1], fp[j]), __dsub_rn(xp[j + 1], xp[j]));
    double r = __dadd_rn(__dmul_rn(slope, __dsub_rn(xq, xp[j])), fp[j]);
    if (r != r) {
        r = __dadd_rn(__dmul_rn(slope, __dsub_rn(xq, xp[j + 1])), fp[j + 1]);
        if (r != r && fp[j] == fp[j + 1]) r = fp[j];
    }
    return r;
}
