// kmpc_sense_faults.hip -- the measurement stage with sensor faults (kmpc_sense_faults_batch), gfx950 only: kmpc_sense_kernel /
// kmpc_sense_delayed_kernel plus outages of the three sources of scripts/state_publisher.py (GPS -> x, y; IMU -> psi; steering report -> v), GPS
// outliers and the publisher's held fixes.  One thread per vehicle, fp64; the vehicle's fault row (16 words) and fault record (16 words) are read
// once and the record written once: about 0.5 KB moved per vehicle and call.  The generator, the ring of truths and the truth-to-estimate arithmetic
// are kmpc_measure.h's (philox4x32_10, sim_delayed_truth, sim_measure: the code the plain kernels' one body calls), so a delivered channel carries
// the bits they give; everything added here is a comparison, a selection or a count (include/kmpc.h states the arithmetic).  No lane reads another
// vehicle's words.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kmpc.h"   // KMPC_SENSOR_*, KMPC_FAULT_*, KMPC_FAULTREC_*
#include "kmpc_dispatch.h"
#include "kmpc_stage.h"
#include "kmpc_measure.h"

#pragma clang fp contract(off)

__global__ __launch_bounds__(256) void kmpc_sense_faults_kernel(int B, const double *__restrict__ state, const double *__restrict__ sensor,
                                                                const double *__restrict__ faults, uint64_t seed, uint64_t period, uint64_t id_base,
                                                                const int32_t *__restrict__ meas_delay, double *truth_ring, int depth,
                                                                double *__restrict__ fault_rec, double *__restrict__ z_out,
                                                                double *__restrict__ held_out, int32_t *__restrict__ flags_out,
                                                                uint8_t *__restrict__ blind_out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    // the vehicle's fault row, record and sensor row, fetched whole before anything is computed: the loads are in flight during the draws
    const double *frow = faults + KMPC_FAULT_WORDS * (size_t)i, *sg = sensor + KMPC_SENSOR_WORDS * (size_t)i;
    double *rec = fault_rec + KMPC_FAULTREC_WORDS * (size_t)i;
    double fr[KMPC_FAULT_WORDS - 1], r[KMPC_FAULTREC_WORDS], sr[KMPC_SENSOR_WORDS];
    for (int k = 0; k < KMPC_FAULT_WORDS - 1; ++k) fr[k] = frow[k];      // word 15 is read by nobody
    for (int k = 0; k < KMPC_FAULTREC_WORDS; ++k) r[k] = rec[k];
    for (int k = 0; k < KMPC_SENSOR_WORDS; ++k) sr[k] = sg[k];
    const double count = r[KMPC_FAULTREC_COUNT], chain_w = r[KMPC_FAULTREC_CHAIN];
    const uint64_t gid = id_base + (uint64_t)i;
    uint32_t w[4], wf[4];
    philox4x32_10((uint32_t)gid, (uint32_t)(gid >> 32), (uint32_t)period, (uint32_t)(period >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), w);
    // the fault draw: the same key, the counter's top bit set -- a period is below 2^63, so no measurement draw has it
    philox4x32_10((uint32_t)gid, (uint32_t)(gid >> 32), (uint32_t)period, (uint32_t)(period >> 32) ^ 0x80000000u, (uint32_t)seed,
                  (uint32_t)(seed >> 32), wf);

    // the truth that is measured: this period's, or with a ring kmpc_sense_delayed_kernel's selection (its ring write included)
    const double *st = state + 8 * (size_t)i;
    double t[4];
    for (int c = 0; c < 4; ++c) t[c] = st[c];
    if (meas_delay) sim_delayed_truth(t, truth_ring, depth, B, i, period, meas_delay);

    const bool chain_ok = chain_w == 0.0 || chain_w == 1.0 || chain_w == 2.0 || chain_w == 3.0 || chain_w == 4.0 || chain_w == 5.0 || chain_w == 6.0 ||
                          chain_w == 7.0;
    const bool reset = !(stage::finite(count) && count >= 0.0) || !chain_ok;
    const bool fresh = reset || count == 0.0;     // a fresh record's other words are not read: they count as zero
    const int was = fresh ? 0 : (int)chain_w;
    if (fresh)
        for (int k = 0; k < KMPC_FAULTREC_WORDS; ++k) r[k] = 0.0;

    const double p = (double)period;
    int chain = 0, silent = 0;
    for (int s = 0; s < 3; ++s) {
        const double u = ((double)wf[s] + 0.5) * 0x1p-32;
        const bool ch = ((was >> s) & 1) ? !(u < fr[KMPC_FAULT_P_REGAIN_GPS + s]) : (u < fr[KMPC_FAULT_P_LOSE_GPS + s]);
        const double from = fr[KMPC_FAULT_WIN_FROM_GPS + s], len = fr[KMPC_FAULT_WIN_LEN_GPS + s];
        const bool sched = len > 0.0 && p >= from && p < from + len;
        if (!fresh && ch) chain |= 1 << s;
        if (!fresh && (ch || sched)) silent |= 1 << s;
    }
    const bool outlier = !fresh && !(silent & 1) && ((double)wf[3] + 0.5) * 0x1p-32 < fr[KMPC_FAULT_P_OUTLIER];

    // the vehicle's sensor row, an outlier fix drawn with OUTLIER_SIGMA on x and y
    const double so = fr[KMPC_FAULT_OUTLIER_SIGMA];
    sr[KMPC_SENSOR_SIGMA_X] = outlier ? so : sr[KMPC_SENSOR_SIGMA_X];
    sr[KMPC_SENSOR_SIGMA_Y] = outlier ? so : sr[KMPC_SENSOR_SIGMA_Y];
    double m[4];
    sim_measure(t, sr, w, m);

    const double max_age = fr[KMPC_FAULT_MAX_AGE];
    const double qnan = __builtin_nan("");
    double z[4];
    bool blind = false;
    for (int c = 0; c < 4; ++c) {
        const int s = c < 2 ? 0 : c - 1;          // x, y: GPS; psi: IMU; v: the steering report
        const bool sil = (silent >> s) & 1;
        z[c] = sil ? qnan : m[c];
        r[KMPC_FAULTREC_HELD_X + c] = sil ? r[KMPC_FAULTREC_HELD_X + c] : m[c];
    }
    for (int s = 0; s < 3; ++s) {
        const bool sil = (silent >> s) & 1;
        const double age = sil ? r[KMPC_FAULTREC_AGE_GPS + s] + 1.0 : 0.0, n0 = r[KMPC_FAULTREC_N_SILENT_GPS + s], lg0 = r[KMPC_FAULTREC_LONGEST_GPS + s];
        r[KMPC_FAULTREC_AGE_GPS + s] = age;
        r[KMPC_FAULTREC_N_SILENT_GPS + s] = sil ? n0 + 1.0 : n0;
        r[KMPC_FAULTREC_LONGEST_GPS + s] = age > lg0 ? age : lg0;
        blind = blind || age > max_age;
    }
    r[KMPC_FAULTREC_N_OUTLIER] = outlier ? r[KMPC_FAULTREC_N_OUTLIER] + 1.0 : r[KMPC_FAULTREC_N_OUTLIER];
    r[KMPC_FAULTREC_COUNT] = r[KMPC_FAULTREC_COUNT] + 1.0;
    r[KMPC_FAULTREC_CHAIN] = (double)chain;
    // one pass of stores: the record whole, then the two views of the measurement
    for (int k = 0; k < KMPC_FAULTREC_WORDS; ++k) rec[k] = r[k];
    for (int c = 0; c < 4; ++c) z_out[4 * (size_t)i + c] = z[c];
    for (int c = 0; c < 4; ++c) held_out[4 * (size_t)i + c] = r[KMPC_FAULTREC_HELD_X + c];
    if (flags_out)
        flags_out[i] = silent | (outlier ? KMPC_FAULT_FLAG_OUTLIER : 0) | (blind ? KMPC_FAULT_FLAG_BLIND : 0) | (fresh ? KMPC_FAULT_FLAG_FRESH : 0) |
                       (reset ? KMPC_FAULT_FLAG_RESET : 0);
    if (blind_out) blind_out[i] = blind ? 1 : 0;
}

hipError_t kmpc_launch_sense_faults(int B, const double *state, const double *sensor, const double *faults, uint64_t seed, uint64_t period,
                                    uint64_t id_base, const int32_t *meas_delay, double *truth_ring, int depth, double *fault_rec, double *z_out,
                                    double *held_out, int32_t *flags_out, uint8_t *blind_out, hipStream_t st)
{
    hipLaunchKernelGGL(kmpc_sense_faults_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, state, sensor, faults, seed, period, id_base, meas_delay,
                       truth_ring, depth, fault_rec, z_out, held_out, flags_out, blind_out);
    return hipGetLastError();
}
