// kmpc_wander.hip -- the Gauss-Markov stage (kmpc_wander_batch), gfx950 only: eight first-order processes per vehicle, advanced once per control
// period and composed into the sensor row's biases and the road row's A_LONG, A_LAT, DF_OFFSET, which the measurement and plant kernels read as
// they always did.  One thread per vehicle, fp64; the vehicle's row (24 words), record (16) and the two base rows (8 + 8) are fetched whole before
// the draws, so the loads are in flight during the Philox rounds, and everything is stored in one pass at the end: about 0.7 KB moved per vehicle
// and call.  The generator is kmpc_measure.h's; include/kmpc.h states the arithmetic.  No lane reads another vehicle's words.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kmpc.h"   // KMPC_WANDER_*, KMPC_WANDERREC_*, KMPC_SENSOR_*, KMPC_ROAD_*
#include "kmpc_dispatch.h"
#include "kmpc_stage.h"
#include "kmpc_measure.h"

#pragma clang fp contract(off)

__global__ __launch_bounds__(256) void kmpc_wander_kernel(int B, const double *__restrict__ wander, double *__restrict__ wander_rec, uint64_t seed,
                                                          uint64_t period, uint64_t id_base, const double *__restrict__ sensor_base,
                                                          double *__restrict__ sensor_out, const double *__restrict__ road_base,
                                                          double *__restrict__ road_out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    constexpr int NC = KMPC_WANDER_CHANNELS;
    const double *row = wander + KMPC_WANDER_WORDS * (size_t)i;
    double *rec = wander_rec + KMPC_WANDERREC_WORDS * (size_t)i;
    double wr[KMPC_WANDER_WORDS], r[KMPC_WANDERREC_WORDS], sr[KMPC_SENSOR_WORDS], rr[KMPC_ROAD_WORDS];
#pragma unroll
    for (int k = 0; k < KMPC_WANDER_WORDS; ++k) wr[k] = row[k];
#pragma unroll
    for (int k = 0; k < KMPC_WANDERREC_WORDS; ++k) r[k] = rec[k];
    if (sensor_out) {
#pragma unroll
        for (int k = 0; k < KMPC_SENSOR_WORDS; ++k) sr[k] = sensor_base[KMPC_SENSOR_WORDS * (size_t)i + k];
    }
    if (road_out) {
#pragma unroll
        for (int k = 0; k < KMPC_ROAD_WORDS; ++k) rr[k] = road_base[KMPC_ROAD_WORDS * (size_t)i + k];
    }

    bool on[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) on[c] = !(wr[KMPC_WANDER_S0 + c] == 0.0 && wr[KMPC_WANDER_Q + c] == 0.0);

    // the normals: call j serves channels 4j ... 4j+3, and a call (a pair) nobody needs is skipped
    const uint64_t gid = id_base + (uint64_t)i;
    double n[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) n[c] = 0.0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (on[4 * j] || on[4 * j + 1] || on[4 * j + 2] || on[4 * j + 3]) {
            uint32_t w[4];
            philox4x32_10((uint32_t)gid, (uint32_t)(gid >> 32), (uint32_t)period, (uint32_t)(period >> 32) ^ (j == 0 ? 0x40000000u : 0xC0000000u),
                          (uint32_t)seed, (uint32_t)(seed >> 32), w);
            if (on[4 * j] || on[4 * j + 1]) box_muller(w[0], w[1], &n[4 * j], &n[4 * j + 1]);
            if (on[4 * j + 2] || on[4 * j + 3]) box_muller(w[2], w[3], &n[4 * j + 2], &n[4 * j + 3]);
        }
    }

    const double count = r[KMPC_WANDERREC_COUNT];
    const bool fresh = !(stage::finite(count) && count >= 0.0) || count == 0.0;   // a fresh record's X words are not read
    double x[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const double first = wr[KMPC_WANDER_S0 + c] * n[c];
        const double carried = wr[KMPC_WANDER_A + c] * r[KMPC_WANDERREC_X + c], fed = wr[KMPC_WANDER_Q + c] * n[c];
        const double next = carried + fed;
        x[c] = on[c] ? (fresh ? first : next) : 0.0;
    }

    // one pass of stores: the record, then the composed rows
#pragma unroll
    for (int c = 0; c < NC; ++c) rec[KMPC_WANDERREC_X + c] = x[c];
    rec[KMPC_WANDERREC_COUNT] = fresh ? 1.0 : count + 1.0;
#pragma unroll
    for (int k = KMPC_WANDERREC_COUNT + 1; k < KMPC_WANDERREC_WORDS; ++k) rec[k] = r[k];
    if (sensor_out) {
        double *o = sensor_out + KMPC_SENSOR_WORDS * (size_t)i;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            o[KMPC_SENSOR_SIGMA_X + c] = sr[KMPC_SENSOR_SIGMA_X + c];
            o[KMPC_SENSOR_BIAS_X + c] = on[c] ? sr[KMPC_SENSOR_BIAS_X + c] + x[c] : sr[KMPC_SENSOR_BIAS_X + c];
        }
    }
    if (road_out) {
        double *o = road_out + KMPC_ROAD_WORDS * (size_t)i;
        rr[KMPC_ROAD_A_LONG] = on[KMPC_WANDER_CH_A_LONG] ? rr[KMPC_ROAD_A_LONG] + x[KMPC_WANDER_CH_A_LONG] : rr[KMPC_ROAD_A_LONG];
        rr[KMPC_ROAD_A_LAT] = on[KMPC_WANDER_CH_A_LAT] ? rr[KMPC_ROAD_A_LAT] + x[KMPC_WANDER_CH_A_LAT] : rr[KMPC_ROAD_A_LAT];
        rr[KMPC_ROAD_DF_OFFSET] = on[KMPC_WANDER_CH_DF_OFFSET] ? rr[KMPC_ROAD_DF_OFFSET] + x[KMPC_WANDER_CH_DF_OFFSET] : rr[KMPC_ROAD_DF_OFFSET];
#pragma unroll
        for (int k = 0; k < KMPC_ROAD_WORDS; ++k) o[k] = rr[k];
    }
}

hipError_t kmpc_launch_wander(int B, const double *wander, double *wander_rec, uint64_t seed, uint64_t period, uint64_t id_base,
                              const double *sensor_base, double *sensor_out, const double *road_base, double *road_out, hipStream_t st)
{
    hipLaunchKernelGGL(kmpc_wander_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, wander, wander_rec, seed, period, id_base, sensor_base,
                       sensor_out, road_base, road_out);
    return hipGetLastError();
}
