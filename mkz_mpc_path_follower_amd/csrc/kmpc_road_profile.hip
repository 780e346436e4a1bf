// kmpc_road_profile.hip -- the road under each vehicle, once per period, on gfx950: a profile with one row per recorded sample of a set of paths
// (grip scale, grade, bank; include/kmpc.h, KMPC_PROFILE_*) composed with the vehicle's own road row into the row the plant reads.
//
// The plant's road (kmpc_sim_advance_road, kmpc_sim_advance_drive) is one row per vehicle for a whole call.  An ice patch in one corner, a bank that
// comes and goes, a grade on one stretch are properties of the PLACE: this stage looks the place up -- the vehicle's nearest recorded sample, with
// nearest_sample (kmpc_nearest.h), the argmin of the waypoint kernel and of the speed plan -- and writes road_out = road_base composed with that
// sample's row.  Piecewise constant by nearest sample: no interpolation (the recorded paths are sampled every 0.24 m, and the plant holds a row for
// one call anyway).
//
// kmpc_road_profile_fleet_kernel: one wavefront per vehicle, as kmpc_waypoints_fleet_kernel; after the argmin lanes 0 ... 7 write the row, one word
// each.  Words 4 ... 7 and the whole row of a refused vehicle are moved, not computed: bit for bit, NaN payloads included.  Arithmetic is one _rn
// operation per word.  Plain C++: vector stores, no LDS, no scratch, no inline assembly.
#include "../../include/kmpc.h"   // KMPC_PROFILE_*, KMPC_ROAD_*: the row layouts
#include "kmpc_common.h"
#include "kmpc_dispatch.h"
#include "kmpc_nearest.h"
#include "kmpc_stage.h"           // stage::finite

#pragma clang fp contract(off)

__global__ __launch_bounds__(64) void kmpc_road_profile_fleet_kernel(RPF w)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= w.B) return;
    const int pid = __builtin_amdgcn_readfirstlane(w.path_id[b]);
    const double *st = w.state + (size_t)b * w.stride, *base = w.road_base + KMPC_ROAD_WORDS * (size_t)b;
    double *out = w.road_out + KMPC_ROAD_WORDS * (size_t)b;
    const double x = uniform_(st[0]), y = uniform_(st[1]);
    // a refused vehicle drives on its own base road; no table entry and no sample is read for a bad path_id, nor for a bad pose
    if (!((unsigned)pid < (unsigned)w.P && stage::finite(x) && stage::finite(y))) {
        if (lane < KMPC_ROAD_WORDS) out[lane] = base[lane];
        if (lane == 0 && w.closest) w.closest[b] = -1;
        return;
    }
    const int o0 = __builtin_amdgcn_readfirstlane(w.off[pid]), o1 = __builtin_amdgcn_readfirstlane(w.off[pid + 1]);
    const size_t n = (size_t)w.total;
    const double *seg = w.d + o0;                                    // d = t | X | Y | psi | s
    const int i = nearest_sample(seg + n, seg + 2 * n, o1 - o0, x, y, lane);   // 0 <= i < M: the row below is inside the vehicle's own path
    const double *r = w.profile + KMPC_PROFILE_WORDS * ((size_t)o0 + (size_t)i);
    if (lane < KMPC_ROAD_WORDS) {
        double v = base[lane];
        if (lane <= KMPC_ROAD_MU_R) v = __dmul_rn(v, r[KMPC_PROFILE_MU_SCALE]);                       // MU_F, MU_R: inf stays inf
        else if (lane == KMPC_ROAD_A_LONG) v = __dadd_rn(v, r[KMPC_PROFILE_A_LONG]);
        else if (lane == KMPC_ROAD_A_LAT) v = __dadd_rn(v, r[KMPC_PROFILE_A_LAT]);
        out[lane] = v;                                                                             // words 4 ... 7: base's bits
    }
    if (lane == 0 && w.closest) w.closest[b] = i;
}

hipError_t kmpc_launch_road_profile_fleet(const RPF &w, hipStream_t st)
{
    return kmpc_launch(kmpc_road_profile_fleet_kernel, dim3(w.B), dim3(64), 0, st, w);
}
