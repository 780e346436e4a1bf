// kmpc_nearest.h -- the nearest recorded sample to a point, by one wavefront: the argmin of the waypoint kernel (kmpc_waypoints.hip), shared with the
// speed plan (kmpc_speed_plan.hip), so that both stages name the same sample for the same pose, bit for bit.
#pragma once
#include "kmpc_common.h"

// argmin over i < M of (X[i]-x)^2 + (Y[i]-y)^2, first occurrence (np.argmin; scripts/gps_utils/ref_gps_traj.py:172): lane l visits samples l, l + 64, ...
// No FMA contraction in the distance, so the index matches numpy's bit for bit.  X, Y, M, x and y are wave-uniform; the result is, too.
DEV int nearest_sample(const double *X, const double *Y, const int M, const double x, const double y, const int lane)
{
    double best = INFINITY;
    int bi = 0x7fffffff;
    for (int i = lane; i < M; i += 64) {
        const double dx = __dsub_rn(X[i], x), dy = __dsub_rn(Y[i], y);
        const double d = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
        if (d < best) { best = d; bi = i; }
    }
    const double dmin = dpp_min(best);
    const double cand = (best == dmin) ? (double)bi : 1e18;
    const int closest = (int)dpp_min(cand);
    // a non-finite pose (NaN or +-inf from the GPS / plant) makes every distance NaN or +inf: no lane records an index.  np.argmin
    // returns 0 then (first NaN / first of the equal minima), and so does this -- never an index outside the path arrays
    return (unsigned)closest < (unsigned)M ? closest : 0;
}
