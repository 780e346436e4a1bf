// kmpc_measure.h -- what the measurement kernels share (kmpc_sim.hip: kmpc_sense_kernel, kmpc_sense_delayed_kernel; kmpc_sense_faults.hip): the
// generator, the ring of truths and the arithmetic from truth to estimate, so that a channel delivered by any of them carries the same bits.
// The normals are a pure function of (seed, id_base + b, period) -- Philox4x32-10 keyed by the seed, counter = (vehicle id, period), Box-Muller
// on the four words (include/kmpc.h has the specification) -- so a vehicle's noise does not depend on B, on the launch geometry or on the shard
// that simulates it.  A channel with sigma == 0 skips the noise term: est = truth + bias bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kmpc.h"   // KMPC_SENSOR_*
#include "kmpc_stage.h"

#pragma clang fp contract(off)

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4])
{
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// two Philox words -> two normals, the operations of sim_measure's pair below (kmpc_wander.hip; sim_measure keeps its own text)
__device__ __forceinline__ void box_muller(uint32_t w0, uint32_t w1, double *n0, double *n1)
{
    const double u0 = ((double)w0 + 0.5) * 0x1p-32, u1 = ((double)w1 + 0.5) * 0x1p-32;
    const double r = sqrt(-2.0 * log(u0)), a = 6.283185307179586 * u1;
    *n0 = r * cos(a);
    *n1 = r * sin(a);
}

// Stale fixes: this period's truth t = x, y, psi, vx goes into slot period mod depth of truth_ring [depth,B,4] (consecutive lanes write consecutive
// 32 B) and t becomes the truth of slot (period - L) mod depth, L = clamp(meas_delay[i], 0, min(depth - 1, period)).
__device__ __forceinline__ void sim_delayed_truth(double t[4], double *truth_ring, int depth, int B, int i, uint64_t period,
                                                  const int32_t *__restrict__ meas_delay)
{
    const size_t slot_words = 4 * (size_t)B;
    double *own = truth_ring + (size_t)(period % (uint64_t)depth) * slot_words + 4 * (size_t)i;
    for (int c = 0; c < 4; ++c) own[c] = t[c];
    const uint64_t lmax = period < (uint64_t)(depth - 1) ? period : (uint64_t)(depth - 1);
    const int lraw = meas_delay[i];
    const uint64_t L = lraw <= 0 ? 0 : ((uint64_t)lraw > lmax ? lmax : (uint64_t)lraw);
    if (L > 0) {
        const double *old = truth_ring + (size_t)((period - L) % (uint64_t)depth) * slot_words + 4 * (size_t)i;
        for (int c = 0; c < 4; ++c) t[c] = old[c];
    }
}

// what the measurement kernels do once the truth t = x, y, psi, vx is fetched and the four Philox words w are drawn: bias, noise, the plant's wrap
// (:101; a heading in range passes unchanged) and the steering report's speed floor
__device__ __forceinline__ void sim_measure(const double t[4], const double *__restrict__ sr, const uint32_t w[4], double *__restrict__ o)
{
    double e[4];
    for (int c = 0; c < 4; ++c) e[c] = t[c] + sr[KMPC_SENSOR_BIAS_X + c];
    for (int h = 0; h < 2; ++h) {
        const double sg0 = sr[KMPC_SENSOR_SIGMA_X + 2 * h], sg1 = sr[KMPC_SENSOR_SIGMA_X + 2 * h + 1];
        if (sg0 != 0.0 || sg1 != 0.0) {
            const double u0 = ((double)w[2 * h] + 0.5) * 0x1p-32, u1 = ((double)w[2 * h + 1] + 0.5) * 0x1p-32;
            const double r = sqrt(-2.0 * log(u0)), a = 6.283185307179586 * u1;
            if (sg0 != 0.0) e[2 * h] = e[2 * h] + sg0 * (r * cos(a));
            if (sg1 != 0.0) e[2 * h + 1] = e[2 * h + 1] + sg1 * (r * sin(a));
        }
    }
    e[2] = stage::wrap(e[2]);
    e[3] = fmax(0.0, e[3]);              // the steering report's speed is not negative
    o[0] = e[0]; o[1] = e[1]; o[2] = e[2]; o[3] = e[3];
}
