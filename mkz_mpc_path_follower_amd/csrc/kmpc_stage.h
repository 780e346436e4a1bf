// kmpc_stage.h -- the scalar helpers the closed loops' stage kernels share (kmpc_sim.hip, kmpc_estimator.hip, kmpc_observer.hip, kmpc_latency.hip):
// one each of the angle wrap, the clip, the finiteness test and the command log's index arithmetic.  The model arithmetic of those units rounds
// operation by operation, so FP contraction is off from here to the end of the including unit (each of them switches it off itself as well).
// The solver units do not include it.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace stage {

// the plant's wrap to [-pi, pi) (vehicle_simulator.py:101: python's float %, the result has the divisor's sign), only where there is something to
// wrap: an angle inside the range passes unchanged, bit for bit
__device__ __forceinline__ double wrap(double a)
{
    const double pi = 3.141592653589793, p2 = 2.0 * pi;
    if (!(a >= -pi && a < pi)) {
        double md = fmod(a + pi, p2);
        if (md < 0.0) md += p2;
        a = md - pi;
    }
    return a;
}

// compare-and-select: inside the cap a keeps its own bits, a NaN passes
__device__ __forceinline__ double clip(double a, double cap) { return a > cap ? cap : (a < -cap ? -cap : a); }

__device__ __forceinline__ bool finite(double a) { return fabs(a) <= 1.7976931348623157e308; }   // false for NaN and +-inf

// floor(a / n) for n > 0, towards -infinity (C's division truncates towards 0)
__device__ __forceinline__ long long floor_div(long long a, long long n) { return a >= 0 ? a / n : -((-a + n - 1) / n); }

// a delay as given, into [lo, hi]
__device__ __forceinline__ int clamp_delay(int v, int lo, long long hi) { return v < lo ? lo : ((long long)v > hi ? (int)hi : v); }

// the command of period j as a log [depth,B,2] has it (slot j mod depth): (0, 0) before the first period (vehicle_simulator.py:21-22)
__device__ __forceinline__ void command(const double *hist, int depth, int B, int i, long long j, double *acc, double *d_f)
{
    *acc = 0.0; *d_f = 0.0;
    if (j >= 0) {
        const double *e = hist + ((size_t)(j % depth) * (size_t)B + (size_t)i) * 2;
        *acc = e[0]; *d_f = e[1];
    }
}

}   // namespace stage
