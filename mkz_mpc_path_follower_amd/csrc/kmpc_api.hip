// kmpc_api.hip -- host side of the C ABI declared in include/kmpc.h (gfx950 / MI355X only).
// The library has no CPU fallback: every entry point that computes launches the HIP kernels
// of kmpc_kernels.hip and fails with KMPC_ERR_NODEVICE / KMPC_ERR_HIP when it cannot.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <chrono>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/kmpc.h"
#include "../../include/kmpc_follow.h"
#include "../../include/kmpc_lanes.h"
#include "../../include/kmpc_range.h"
#include "../../include/kmpc_order.h"
#include "kmpc_dispatch.h"

#ifndef KMPC_HOST_ZERO_COPY_MAX
#define KMPC_HOST_ZERO_COPY_MAX 16   // kmpc_solve_batch_host: batches up to this size run on pinned host memory (no copies); above, staged through device memory
#endif

struct kmpc_handle {
    kmpc_config cfg = {};
    int device = 0;
    hipStream_t stream = nullptr;
    double cost[8] = {};
    std::string err;
    // staging for the host-pointer entry point
    void *dbuf = nullptr;
    size_t dbuf_bytes = 0;
    // ... and for SMALL batches (B <= KMPC_HOST_ZERO_COPY_MAX: the reference's own B = 1 loop) one pinned, device-mapped host buffer the kernel reads its
    // inputs from and writes its outputs to directly: no copy launches at all (round 4: 13 small pageable copies cost 120 us of a 174 us control step)
    void *hbuf = nullptr, *hbuf_dev = nullptr;
    size_t hbuf_bytes = 0;
    unsigned int *done_flag = nullptr;   // device view of the completion counter inside hbuf while such a launch is being issued, else NULL
    // start-order workspace (kmpc_schedule.hip): perm[cap], tag[cap], hist[2][256]
    int32_t *perm = nullptr;
    uint32_t *tag = nullptr, *hist = nullptr;
    size_t sched_cap = 0;
    unsigned sched_parity = 0;
};

static std::string g_create_err;
static unsigned long long *g_stamps = nullptr;  // set by kmpc_debug_set_stamps in diagnostic builds
#if defined(KMPC_STAMPS) || defined(KMPC_TRACE)
extern "C" int32_t kmpc_debug_set_stamps(void *p) { g_stamps = (unsigned long long *)p; return 0; }
#endif

static int fail(kmpc_handle *h, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_err = buf;
    return code;
}

#define HIPCHK(h, call)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) return fail(h, KMPC_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

extern "C" int32_t kmpc_abi_version(void) { return KMPC_ABI_VERSION; }

// MKZMPCPathFollower.jl:28-48
extern "C" int32_t kmpc_config_default(kmpc_config *c, int32_t N, int32_t dtype)
{
    if (!c) return KMPC_ERR_ARG;
    memset(c, 0, sizeof *c);
    c->N = N;
    c->dtype = dtype;
    c->dt = 0.20;
    c->dt_control = 0.10;
    c->L_a = 1.108;
    c->L_b = 1.742;
    c->steer_max = 0.5;
    c->steer_dmax = 0.5;
    c->a_max = 1.0;
    c->a_dmax = 1.5;
    c->v_min = 0.0;
    c->v_max = 20.0;
    c->max_iter = 200;
    c->hessian = 1;
    c->tol = dtype == KMPC_F32 ? 1e-4 : 1e-8;
    c->mu_init = 1.0;  // Ipopt default is 0.1; with the objective scaled to max-gradient 100, mu = 1 centres the first iterates better (mean iterations -5 %, thinner tail)
    c->bound_relax = dtype == KMPC_F32 ? 1e-5 : 1e-8;
    c->warm_push = 1e-5;  // (1e-5, 1e-6): closed loop on the recorded path 5.5 / 5.0 -> 4.4 / 4.4 mean iterations against (1e-4, 1e-6); a warm start from the solution of an UNRELATED problem is still always Optimal (tools/warm_probe.py, tools/closed_loop_probe.py)
    c->warm_mu = 1e-6;
    c->max_ls = 30;
    c->indef_strategy = 2;  // indefinite exact Hessian: hybrid (Gauss-Newton fallback, delta_w shift from the second failure on)
    c->schedule = 1;  // longest-predicted-first start order (kmpc_schedule.hip)
    c->model = 0;
    c->mu_strategy = 1;  // Mehrotra predictor-corrector (all Optimal on seeded draws at N = 8 ... 56; a third fewer iterations than the monotone rule)
    c->start = 0;        // feed-forward start (1 = the reference's all-zero start, MKZMPCPathFollower.jl:65-72)
    return KMPC_OK;
}

extern "C" int32_t kmpc_create(const kmpc_config *cfg, int32_t device, kmpc_handle **out)
{
    if (!cfg || !out) return fail(nullptr, KMPC_ERR_ARG, "kmpc_create: null argument");
    if (cfg->N < 2 || cfg->N > 56) return fail(nullptr, KMPC_ERR_ARG, "kmpc_create: horizon N=%d outside 2..56", cfg->N);
    if (cfg->dtype != KMPC_F64 && cfg->dtype != KMPC_F32) return fail(nullptr, KMPC_ERR_ARG, "kmpc_create: bad dtype %d", cfg->dtype);
    if (!(cfg->dt > 0) || !(cfg->dt_control > 0) || !(cfg->L_b > 0) || !(cfg->L_a + cfg->L_b > 0) ||
        !(cfg->v_max > cfg->v_min) || !(cfg->a_max > 0) || !(cfg->steer_max > 0) || !(cfg->steer_max < 1.5) ||
        !(cfg->a_dmax > 0) || !(cfg->steer_dmax > 0) || cfg->max_iter < 1 || cfg->max_ls < 1 || !(cfg->tol > 0) ||
        cfg->kernel_variant < 0 || cfg->kernel_variant > 3 || cfg->mu_strategy < 0 || cfg->mu_strategy > 1 ||
        cfg->indef_strategy < 0 || cfg->indef_strategy > 2 || cfg->schedule < 0 || cfg->schedule > 1 || cfg->model < 0 || cfg->model > 1 ||
        cfg->start < 0 || cfg->start > 1)
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_create: invalid model / solver parameter");
    // a configuration is accepted exactly when kmpc_select (kmpc_dispatch.h) has a kernel for it; what follows only words the refusal
    if (!kmpc_selectable(cfg->model, cfg->kernel_variant, cfg->N, cfg->dtype == KMPC_F64)) {
        const bool compiled = kmpc_in(kmpc_fast_horizons(), cfg->N) || kmpc_in(kmpc_wide_horizons(), cfg->N);
        if (cfg->model == 1 && cfg->N > KMPC_GENERIC_FRENET_MAX_N && (cfg->kernel_variant == 1 || !compiled))   // Frenet beyond the generic kernel's horizons
            return fail(nullptr, KMPC_ERR_ARG, "kmpc_create: invalid model / solver parameter");
        if (cfg->kernel_variant == 3 && cfg->model != 1)   // four Frenet problems per wave (kmpc_quad.hip): model 1 at its reference's horizon only
            return fail(nullptr, KMPC_ERR_ARG, "kmpc_create: kernel_variant = 3 is the four-per-wave Frenet kernel (model = 1); for the Cartesian model "
                        "kernel_variant = 0 picks the four-per-wave kernel by batch size (its padding rows are not gated against the host entry point's completion count)");
        if (cfg->kernel_variant == 3)   // (both precisions: the fp32 instantiation passed its acceptance run, tests/test_frenet_quad.py::test_frenet_quad_fp32_acceptance)
            return fail(nullptr, KMPC_ERR_ARG, "kmpc_create: kernel_variant = 3 needs N = 8 (no four-per-wave Frenet kernel at N = %d)", cfg->N);
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_create: the Frenet model (model = 1) at N = %d runs in fp64 only (no fp32 four-wave Frenet kernel)", cfg->N);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, KMPC_ERR_NODEVICE, "kmpc_create: no HIP device");
    if (device < 0 || device >= ndev) return fail(nullptr, KMPC_ERR_ARG, "kmpc_create: device %d of %d", device, ndev);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(nullptr, KMPC_ERR_HIP, "hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, KMPC_ERR_NODEVICE, "kmpc_create: device %d is %s, this library is built for gfx950 only", device, prop.gcnArchName);
    kmpc_handle *h = new kmpc_handle();
    h->cfg = *cfg;
    h->device = device;
    const double w0[8] = {9.0, 9.0, 10.0, 0.0, 100.0, 1000.0, 0.0, 0.0};  // MKZMPCPathFollower.jl:51-59
    const double w1[8] = {0.0, 9.0, 10.0, 0.5, 100.0, 1000.0, 0.0, 0.0};  // MKZMPCPathFollowerFrenet.jl:51-59 (no x slot)
    memcpy(h->cost, cfg->model == 1 ? w1 : w0, sizeof w0);
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return fail(nullptr, KMPC_ERR_HIP, "kmpc_create: cannot create stream on device %d", device);
    }
    *out = h;
    return KMPC_OK;
}

extern "C" int32_t kmpc_destroy(kmpc_handle *h)
{
    if (!h) return KMPC_OK;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    if (h->dbuf) (void)hipFree(h->dbuf);
    if (h->hbuf) (void)hipHostFree(h->hbuf);
    if (h->perm) (void)hipFree(h->perm);
    if (h->tag) (void)hipFree(h->tag);
    if (h->hist) (void)hipFree(h->hist);
    (void)hipStreamDestroy(h->stream);
    delete h;
    return KMPC_OK;
}

extern "C" int32_t kmpc_set_cost(kmpc_handle *h, const double w[8])
{
    if (!h || !w) return KMPC_ERR_ARG;
    for (int i = 0; i < 8; ++i)
        if (!(w[i] >= 0.0)) return fail(h, KMPC_ERR_ARG, "kmpc_set_cost: weight %d is negative or NaN", i);
    memcpy(h->cost, w, 8 * sizeof(double));
    return KMPC_OK;
}

extern "C" int32_t kmpc_get_cost(kmpc_handle *h, double w[8])
{
    if (!h || !w) return KMPC_ERR_ARG;
    memcpy(w, h->cost, 8 * sizeof(double));
    return KMPC_OK;
}

extern "C" const char *kmpc_last_error(kmpc_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }

static KP make_kp(const kmpc_handle *h, int B, int warm, int hessian_override)
{
    const kmpc_config &c = h->cfg;
    KP P;
    memset(&P, 0, sizeof P);
    P.N = c.N; P.B = B; P.max_iter = c.max_iter;
    P.hessian = hessian_override >= 0 ? hessian_override : c.hessian;
    P.warm = warm; P.max_ls = c.max_ls; P.mu_strategy = c.mu_strategy; P.indef_strategy = c.indef_strategy;
    P.start = c.start;
    P.dt = c.dt; P.dtc = c.dt_control; P.L_b = c.L_b; P.r = c.L_b / (c.L_a + c.L_b);
    P.steer_max = c.steer_max; P.steer_dmax = c.steer_dmax; P.a_max = c.a_max; P.a_dmax = c.a_dmax;
    P.v_min = c.v_min; P.v_max = c.v_max;
    memcpy(P.C, h->cost, sizeof P.C);
    P.tol = c.tol; P.mu_init = c.mu_init; P.relax = c.bound_relax; P.warm_push = c.warm_push; P.warm_mu = c.warm_mu;
    P.gap_tol = c.dtype == KMPC_F32 ? 1e-4 : 1e-7;  // unscaled duality-gap bound relative to max(1, |J|)
    for (int i = 0; i < 8; ++i) P.C2[i] = 2.0 * P.C[i];
    P.dt2 = P.dt * P.dt; P.dt_over_Lb = P.dt / P.L_b;
    P.tol_x100 = 100.0 * P.tol; P.tol_x1000 = 1e3 * P.tol; P.tol_d100 = P.tol * 1e-2; P.tol_d10 = P.tol / 10.0;
    return P;
}

// input record of kmpc_solve_batch_packed in scalars: z0[4], v_target, u_prev[2], pad, ref[(N+1)*3], rounded up to whole 64-B lines (72 scalars
// = 576 B at N = 20, fp64).  (Whole 128-B lines were measured too: same counter traffic, more padding -- profiles/README.md, round 4.)
static inline int record_scalars(int N, int dtype)
{
    const int per_line = dtype == KMPC_F64 ? 8 : 16;
    return (8 + 3 * (N + 1) + per_line - 1) / per_line * per_line;
}

// the buffers of one solve call as the C entry points receive them (element type: the handle's); rec / orec set = packed records, the arrays unused
struct SolveBuffers {
    const void *z0, *ref, *vt, *up, *par;
    void *warmU;
    int warm;
    void *u0;
    int32_t *status;
    void *cost, *viol;
    int32_t *iters;
    void *outU, *outX;
    const void *rec;
    void *orec;
};

template <typename T>
static int solve_dev(kmpc_handle *h, int B, const SolveBuffers &a, hipStream_t st)
{
    const kmpc_config &c = h->cfg;
    KIO<T> io;
    io.par = (const T *)a.par;   // per-problem weights and limits [B,16] (kmpc_solve_batch_params), NULL = the handle's
    if (a.rec) {   // packed records: the same pointers aim into the records, every stride is the record's
        const T *rec = (const T *)a.rec;
        T *orec = (T *)a.orec;
        io.z0 = rec; io.ref = rec + 8; io.vt = rec + 4; io.up = rec + 5;
        io.zs = io.rs = io.vs = io.us = record_scalars(c.N, c.dtype);
        io.u0 = orec; io.cost = orec + 2; io.viol = orec + 3; io.status = (int32_t *)(orec + 4); io.iters = io.status + 1;
        io.u0s = io.ss = (int)(64 / sizeof(T)); io.is = 16;
    } else {
        io.z0 = (const T *)a.z0; io.ref = (const T *)a.ref; io.vt = (const T *)a.vt; io.up = (const T *)a.up;
        io.zs = 4; io.rs = c.model == 1 ? 4 : 3 * (c.N + 1); io.vs = 1; io.us = 2;
        io.u0 = (T *)a.u0; io.cost = (T *)a.cost; io.viol = (T *)a.viol; io.status = a.status; io.iters = a.iters;
        io.u0s = 2; io.ss = 1; io.is = 1;
    }
    io.warmU = (T *)a.warmU; io.outU = (T *)a.outU; io.outX = (T *)a.outX;
    io.stamps = g_stamps;
    const KP P = make_kp(h, B, a.warm && a.warmU ? 1 : 0, -1);
    io.perm = nullptr;
    io.done = h->done_flag;   // (set only around the small-batch host entry point's launch)
    // start order: only matters once a launch no longer fits on the chip at once.  Cartesian model only: the Frenet functor's `ref` carries k_poly [B,4],
    // and the start-order key reads reference points
    if (c.model == 0 && c.schedule == 1 && B > KMPC_CHIP_FILL_BATCH) {
        if ((size_t)B > h->sched_cap) {
            if (h->perm) (void)hipFree(h->perm);
            if (h->tag) (void)hipFree(h->tag);
            h->perm = nullptr; h->tag = nullptr; h->sched_cap = 0;
            const size_t cap = (size_t)B + (size_t)B / 4;
            HIPCHK(h, hipMalloc((void **)&h->perm, cap * sizeof(int32_t)));
            HIPCHK(h, hipMalloc((void **)&h->tag, cap * sizeof(uint32_t)));
            h->sched_cap = cap;
        }
        if (!h->hist) {
            HIPCHK(h, hipMalloc((void **)&h->hist, 2 * 256 * sizeof(uint32_t)));
            HIPCHK(h, hipMemsetAsync(h->hist, 0, 2 * 256 * sizeof(uint32_t), st));
            h->sched_parity = 0;
        }
        uint32_t *hc = h->hist + 256 * (h->sched_parity & 1), *hn = h->hist + 256 * ((h->sched_parity & 1) ^ 1);
        HIPCHK(h, kmpc_launch_schedule<T>(B, P.N, P.dt, io.z0, (size_t)io.zs, io.ref, (size_t)io.rs, hc, hn, h->tag, h->perm, st));
        h->sched_parity ^= 1;
        io.perm = h->perm;
    }
    const kmpc_selection sel = kmpc_select(c.model, c.kernel_variant, P.N, sizeof(T) == 8, B);
    switch (sel.backend) {
        case KMPC_BACKEND_QUAD: HIPCHK(h, kmpc_launch_solve_quad<T>(P, io, c.model, st)); break;
        case KMPC_BACKEND_FAST: HIPCHK(h, kmpc_launch_solve_fast<T>(P, io, c.model, sel.dense, st)); break;
        case KMPC_BACKEND_WIDE: HIPCHK(h, kmpc_launch_solve_wide<T>(P, io, c.model, st)); break;
        case KMPC_BACKEND_GENERIC: HIPCHK(h, kmpc_launch_solve<T>(P, io, c.model, st)); break;
        case KMPC_BACKEND_NONE: return fail(h, KMPC_ERR_ARG, "no kernel for this configuration");   // (kmpc_create refuses such a handle)
    }
    return KMPC_OK;
}

// what the kmpc_solve_batch* entry points share; `fn` is the entry point's name, `wrong_model` what it says to a handle of the other model
static int solve_entry(kmpc_handle *h, const char *fn, int model, const char *wrong_model, int B, const SolveBuffers &a, void *stream)
{
    if (!h) return KMPC_ERR_ARG;
    if (B < 0) return fail(h, KMPC_ERR_ARG, "%s: B=%d", fn, B);
    if (B == 0) return KMPC_OK;
    const bool packed = a.rec || a.orec;   // (a packed call without either has no arrays either)
    if (packed ? !a.rec || !a.orec : !a.z0 || !a.ref || !a.vt || !a.up || !a.u0 || !a.status)
        return fail(h, KMPC_ERR_ARG, "%s: null required buffer", fn);
    if (((uintptr_t)a.rec | (uintptr_t)a.orec) & 63) return fail(h, KMPC_ERR_ARG, "%s: records must be 64-byte aligned", fn);
    if (h->cfg.model != model) return fail(h, KMPC_ERR_ARG, "%s: %s", fn, wrong_model);
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;  // NULL = the device's default stream, as in HIP
    return h->cfg.dtype == KMPC_F64 ? solve_dev<double>(h, B, a, st) : solve_dev<float>(h, B, a, st);
}

extern "C" int32_t kmpc_solve_batch_params(kmpc_handle *h, int32_t B, const void *z0, const void *ref, const void *v_target,
                                           const void *u_prev, const void *params, void *warm_U, int32_t warm, void *out_u0,
                                           int32_t *out_status, void *out_cost, void *out_viol, int32_t *out_iters, void *out_U,
                                           void *out_X, void *stream)
{
    const SolveBuffers a = {z0, ref, v_target, u_prev, params, warm_U, warm, out_u0, out_status, out_cost, out_viol, out_iters, out_U, out_X, nullptr, nullptr};
    if (!params) return solve_entry(h, "kmpc_solve_batch", 0, "handle was created for the Frenet model; use kmpc_solve_batch_frenet", B, a, stream);
    return solve_entry(h, "kmpc_solve_batch_params", 0, "handle was created for the Frenet model; use kmpc_solve_batch_frenet_params", B, a, stream);
}

extern "C" int32_t kmpc_solve_batch(kmpc_handle *h, int32_t B, const void *z0, const void *ref, const void *v_target,
                                    const void *u_prev, void *warm_U, int32_t warm, void *out_u0, int32_t *out_status,
                                    void *out_cost, void *out_viol, int32_t *out_iters, void *out_U, void *out_X,
                                    void *stream)
{
    return kmpc_solve_batch_params(h, B, z0, ref, v_target, u_prev, nullptr, warm_U, warm, out_u0, out_status, out_cost, out_viol, out_iters, out_U, out_X, stream);
}

extern "C" int32_t kmpc_solve_batch_frenet_params(kmpc_handle *h, int32_t B, const void *z0, const void *k_poly, const void *v_target,
                                                  const void *u_prev, const void *params, void *warm_U, int32_t warm, void *out_u0,
                                                  int32_t *out_status, void *out_cost, void *out_viol, int32_t *out_iters, void *out_U,
                                                  void *out_X, void *stream)
{
    const SolveBuffers a = {z0, k_poly, v_target, u_prev, params, warm_U, warm, out_u0, out_status, out_cost, out_viol, out_iters, out_U, out_X, nullptr, nullptr};
    return solve_entry(h, params ? "kmpc_solve_batch_frenet_params" : "kmpc_solve_batch_frenet", 1, "handle was created with cfg.model = 0", B, a, stream);
}

extern "C" int32_t kmpc_solve_batch_frenet(kmpc_handle *h, int32_t B, const void *z0, const void *k_poly, const void *v_target,
                                           const void *u_prev, void *warm_U, int32_t warm, void *out_u0, int32_t *out_status,
                                           void *out_cost, void *out_viol, int32_t *out_iters, void *out_U, void *out_X,
                                           void *stream)
{
    return kmpc_solve_batch_frenet_params(h, B, z0, k_poly, v_target, u_prev, nullptr, warm_U, warm, out_u0, out_status, out_cost, out_viol, out_iters, out_U, out_X, stream);
}

// MKZMPCPathFollower.jl:158-169 (update_cost) and :41-48 (the limits), as one record per problem
extern "C" int32_t kmpc_get_problem_params(kmpc_handle *h, double rec[16])
{
    if (!h || !rec) return KMPC_ERR_ARG;
    const kmpc_config &c = h->cfg;
    memcpy(rec, h->cost, 8 * sizeof(double));
    rec[8] = c.steer_max; rec[9] = c.steer_dmax; rec[10] = c.a_max; rec[11] = c.a_dmax; rec[12] = c.v_min; rec[13] = c.v_max;
    rec[14] = rec[15] = 0.0;
    return KMPC_OK;
}

extern "C" int64_t kmpc_record_bytes(int32_t N, int32_t dtype)
{
    if (N < 2 || N > 56 || (dtype != KMPC_F64 && dtype != KMPC_F32)) return -1;
    return (int64_t)record_scalars(N, dtype) * (dtype == KMPC_F64 ? 8 : 4);
}

extern "C" int32_t kmpc_pack_records(kmpc_handle *h, int32_t B, const void *z0, const void *ref, const void *v_target, const void *u_prev,
                                     void *records, void *stream)
{
    if (!h) return KMPC_ERR_ARG;
    if (B < 0) return fail(h, KMPC_ERR_ARG, "kmpc_pack_records: B=%d", B);
    if (B == 0) return KMPC_OK;
    if (!z0 || !ref || !v_target || !u_prev || !records) return fail(h, KMPC_ERR_ARG, "kmpc_pack_records: null buffer");
    if (h->cfg.model != 0) return fail(h, KMPC_ERR_ARG, "kmpc_pack_records: Cartesian model only");
    HIPCHK(h, hipSetDevice(h->device));
    const int stride = record_scalars(h->cfg.N, h->cfg.dtype);
    if (h->cfg.dtype == KMPC_F64)
        HIPCHK(h, kmpc_launch_pack<double>(B, h->cfg.N, stride, (const double *)z0, (const double *)ref, (const double *)v_target, (const double *)u_prev, (double *)records, (hipStream_t)stream));
    else
        HIPCHK(h, kmpc_launch_pack<float>(B, h->cfg.N, stride, (const float *)z0, (const float *)ref, (const float *)v_target, (const float *)u_prev, (float *)records, (hipStream_t)stream));
    return KMPC_OK;
}

extern "C" int32_t kmpc_solve_batch_packed(kmpc_handle *h, int32_t B, const void *records, void *warm_U, int32_t warm, void *out_records,
                                           void *out_U, void *out_X, void *stream)
{
    SolveBuffers a = {};
    a.warmU = warm_U; a.warm = warm; a.outU = out_U; a.outX = out_X; a.rec = records; a.orec = out_records;
    return solve_entry(h, "kmpc_solve_batch_packed", 0, "Cartesian model only", B, a, stream);
}

// kmpc_solve_batch_host: the 12 arrays of one batch in one allocation, inputs then outputs, each 256-B aligned
enum { HB_Z0, HB_REF, HB_VT, HB_UP, HB_WARM, HB_U0, HB_STATUS, HB_COST, HB_VIOL, HB_ITERS, HB_OUTU, HB_OUTX, HB_ARRAYS };
struct HostLayout {
    size_t sz[HB_ARRAYS], off[HB_ARRAYS], total;
};
static HostLayout host_layout(size_t b, size_t N, size_t es)
{
    HostLayout L = {{b * 4 * es, b * (N + 1) * 3 * es, b * es, b * 2 * es, b * N * 2 * es,
                     b * 2 * es, b * 4, b * es, b * es, b * 4, b * N * 2 * es, b * (N + 1) * 4 * es}, {}, 0};
    for (int i = 0; i < HB_ARRAYS; ++i) { L.off[i] = L.total; L.total += (L.sz[i] + 255) & ~(size_t)255; }
    return L;
}

extern "C" int32_t kmpc_solve_batch_host(kmpc_handle *h, int32_t B, const void *z0, const void *ref,
                                         const void *v_target, const void *u_prev, void *warm_U, int32_t warm,
                                         void *out_u0, int32_t *out_status, void *out_cost, void *out_viol,
                                         int32_t *out_iters, void *out_U, void *out_X)
{
    if (!h) return KMPC_ERR_ARG;
    if (B < 0) return fail(h, KMPC_ERR_ARG, "kmpc_solve_batch_host: B=%d", B);
    if (B == 0) return KMPC_OK;
    if (!z0 || !ref || !v_target || !u_prev || !out_u0 || !out_status)
        return fail(h, KMPC_ERR_ARG, "kmpc_solve_batch_host: null required buffer");
    if (h->cfg.model != 0) return fail(h, KMPC_ERR_ARG, "kmpc_solve_batch_host: Cartesian model only (use kmpc_solve_batch_frenet with device buffers)");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t es = h->cfg.dtype == KMPC_F64 ? 8 : 4;
    const HostLayout L = host_layout((size_t)B, (size_t)h->cfg.N, es);
    // copy-in: the four inputs, and the warm start when it is used; copy-out, in this order: the outputs the caller asked for, then the warm start
    const void *in[5] = {z0, ref, v_target, u_prev, warm_U && warm ? warm_U : nullptr};
    const int out_slot[8] = {HB_U0, HB_STATUS, HB_COST, HB_VIOL, HB_ITERS, HB_OUTU, HB_OUTX, HB_WARM};
    void *out[8] = {out_u0, out_status, out_cost, out_viol, out_iters, out_U, out_X, warm_U};
    hipStream_t st = h->stream;
    auto solve_at = [&](char *d) {   // d: the allocation as the device sees it
        return kmpc_solve_batch(h, B, d + L.off[HB_Z0], d + L.off[HB_REF], d + L.off[HB_VT], d + L.off[HB_UP], warm_U ? d + L.off[HB_WARM] : nullptr, warm,
                                d + L.off[HB_U0], (int32_t *)(d + L.off[HB_STATUS]), d + L.off[HB_COST], d + L.off[HB_VIOL], (int32_t *)(d + L.off[HB_ITERS]),
                                out_U ? d + L.off[HB_OUTU] : nullptr, out_X ? d + L.off[HB_OUTX] : nullptr, st);
    };
    if (B <= KMPC_HOST_ZERO_COPY_MAX) {
        // small batch: the kernel works on pinned host memory (inputs: one burst of loads per problem when it starts; outputs: posted writes when it ends)
        if (L.total > h->hbuf_bytes) {
            if (h->hbuf) HIPCHK(h, hipHostFree(h->hbuf));
            h->hbuf = h->hbuf_dev = nullptr; h->hbuf_bytes = 0;
            // sized once for the largest zero-copy batch of this handle's horizon, + the completion counter
            const size_t cap = host_layout(KMPC_HOST_ZERO_COPY_MAX, (size_t)h->cfg.N, es).total + 256;
            HIPCHK(h, hipHostMalloc(&h->hbuf, cap, hipHostMallocMapped));
            HIPCHK(h, hipHostGetDevicePointer(&h->hbuf_dev, h->hbuf, 0));
            h->hbuf_bytes = cap;
        }
        char *hp = (char *)h->hbuf, *dp = (char *)h->hbuf_dev;
        for (int i = 0; i < 5; ++i)
            if (in[i]) memcpy(hp + L.off[i], in[i], L.sz[i]);
        // completion: every problem adds 1 to a counter in the pinned buffer after its outputs (release, system scope); the host spins on it -- the runtime's
        // own completion path (interrupt / signal wait) is several microseconds slower -- and falls back to the stream after 2 ms (long solves, stalled device)
        volatile unsigned int *flag_h = (volatile unsigned int *)(hp + h->hbuf_bytes - 256);
        *flag_h = 0u;
        h->done_flag = (unsigned int *)(dp + h->hbuf_bytes - 256);
        int rc = solve_at(dp);
        h->done_flag = nullptr;
        if (rc != KMPC_OK) return rc;
        {
            const auto t0 = std::chrono::steady_clock::now();
            unsigned spins = 0;
            bool seen = false;
            for (;;) {
                if (__atomic_load_n((const unsigned int *)flag_h, __ATOMIC_ACQUIRE) >= (unsigned)B) { seen = true; break; }
                if ((++spins & 1023u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
            }
            if (!seen) HIPCHK(h, hipStreamSynchronize(st));
        }
        for (int i = 0; i < 8; ++i)
            if (out[i]) memcpy(out[i], hp + L.off[out_slot[i]], L.sz[out_slot[i]]);
        return KMPC_OK;
    }
    if (L.total > h->dbuf_bytes) {
        if (h->dbuf) HIPCHK(h, hipFree(h->dbuf));
        h->dbuf = nullptr; h->dbuf_bytes = 0;
        HIPCHK(h, hipMalloc(&h->dbuf, L.total));
        h->dbuf_bytes = L.total;
    }
    char *d = (char *)h->dbuf;
    for (int i = 0; i < 5; ++i)
        if (in[i]) HIPCHK(h, hipMemcpyAsync(d + L.off[i], in[i], L.sz[i], hipMemcpyHostToDevice, st));
    int rc = solve_at(d);
    if (rc != KMPC_OK) return rc;
    for (int i = 0; i < 8; ++i)
        if (out[i]) HIPCHK(h, hipMemcpyAsync(out[i], d + L.off[out_slot[i]], L.sz[out_slot[i]], hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return KMPC_OK;
}

extern "C" int32_t kmpc_debug_condense(kmpc_handle *h, int32_t B, const void *z0, const void *ref, const void *v_target,
                                       const void *U, int32_t hessian, void *H, void *g, void *J, void *stream)
{
    if (!h || B <= 0 || !z0 || !ref || !v_target || !U || !H || !g || !J) return h ? fail(h, KMPC_ERR_ARG, "kmpc_debug_condense: bad argument") : KMPC_ERR_ARG;
    const int model = h->cfg.model;
    if (model == 1 && h->cfg.N > KMPC_GENERIC_FRENET_MAX_N)
        return fail(h, KMPC_ERR_ARG, "kmpc_debug_condense: the generic kernel's Frenet functor is built for N <= %d (N=%d)", KMPC_GENERIC_FRENET_MAX_N, h->cfg.N);
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;  // NULL = the device's default stream, as in HIP
    const KP P = make_kp(h, B, 0, hessian);
    if (h->cfg.dtype == KMPC_F64) {
        KDbg<double> io = {(const double *)z0, (const double *)ref, (const double *)v_target, (const double *)U,
                           (double *)H, (double *)g, (double *)J};
        HIPCHK(h, model == 1 ? kmpc_launch_condense_frenet<double>(P, io, st) : kmpc_launch_condense<double>(P, io, st));
    } else {
        KDbg<float> io = {(const float *)z0, (const float *)ref, (const float *)v_target, (const float *)U,
                          (float *)H, (float *)g, (float *)J};
        HIPCHK(h, model == 1 ? kmpc_launch_condense_frenet<float>(P, io, st) : kmpc_launch_condense<float>(P, io, st));
    }
    return KMPC_OK;
}

template <typename T>
static int debug_kkt(kmpc_handle *h, int B, const void *z0, const void *ref, const void *vt, const void *up, const void *U, const void *w,
                     const void *b, double sc, double reg, int hessian, void *K, void *g, void *x, int32_t *ok, hipStream_t st)
{
    const KP P = make_kp(h, B, 0, hessian);
    KDbgK<T> io = {(const T *)z0, (const T *)ref, (const T *)vt, (const T *)up, (const T *)U, (const T *)w, (const T *)b, sc, reg,
                   (T *)K, (T *)g, (T *)x, ok};
    // the kernel a solve of this handle at this B would run; where that is the generic one (which has no in-register KKT pipeline), the
    // compile-time-horizon kernel of this N (kernel_variant = 2: neither the generic nor the four-per-wave kernel)
    const int model = h->cfg.model;
    kmpc_backend backend = kmpc_select(model, h->cfg.kernel_variant, P.N, sizeof(T) == 8, B).backend;
    if (backend == KMPC_BACKEND_GENERIC) backend = kmpc_select(model, 2, P.N, sizeof(T) == 8, B).backend;
    if (backend == KMPC_BACKEND_FAST) HIPCHK(h, model == 1 ? kmpc_launch_fast_kkt_frenet<T>(P, io, st) : kmpc_launch_fast_kkt<T>(P, io, st));
    else if (backend == KMPC_BACKEND_WIDE) {
        if constexpr (sizeof(T) == 8) HIPCHK(h, model == 1 ? kmpc_launch_wide_kkt_frenet(P, io, st) : kmpc_launch_wide_kkt<T>(P, io, st));
        else HIPCHK(h, kmpc_launch_wide_kkt<T>(P, io, st));   // (kmpc_select has no fp32 four-wave answer for the Frenet model)
    }
    else if (backend == KMPC_BACKEND_QUAD) HIPCHK(h, kmpc_launch_quad_kkt<T>(P, io, model, st));
    else if (model == 1 && sizeof(T) != 8 && kmpc_in(kmpc_wide_horizons(), P.N))
        return fail(h, KMPC_ERR_ARG, "kmpc_debug_kkt: the Frenet model (model = 1) at N=%d runs in fp64 only (no fp32 four-wave Frenet kernel)", P.N);
    else return fail(h, KMPC_ERR_ARG, "kmpc_debug_kkt: no compile-time-horizon kernel for N=%d in this element type", P.N);
    return KMPC_OK;
}

extern "C" int32_t kmpc_debug_kkt(kmpc_handle *h, int32_t B, const void *z0, const void *ref, const void *v_target, const void *u_prev,
                                  const void *U, const void *w, const void *b, double sc, double reg, int32_t hessian, void *K_out,
                                  void *g, void *x, int32_t *ok, void *stream)
{
    if (!h || B <= 0 || !z0 || !ref || !v_target || !u_prev || !U || !w || !b || !K_out || !g || !x || !ok || !(sc > 0) || !(reg >= 0))
        return h ? fail(h, KMPC_ERR_ARG, "kmpc_debug_kkt: bad argument") : KMPC_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    if (h->cfg.dtype == KMPC_F64) return debug_kkt<double>(h, B, z0, ref, v_target, u_prev, U, w, b, sc, reg, hessian, K_out, g, x, ok, st);
    return debug_kkt<float>(h, B, z0, ref, v_target, u_prev, U, w, b, sc, reg, hessian, K_out, g, x, ok, st);
}

extern "C" int32_t kmpc_debug_mfma_probe(kmpc_handle *h, const void *a, const void *b, void *d, void *stream)
{
    if (!h || !a || !b || !d) return KMPC_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;  // NULL = the device's default stream, as in HIP
    if (h->cfg.dtype == KMPC_F64) HIPCHK(h, kmpc_launch_probe<double>((const double *)a, (const double *)b, (double *)d, st));
    else HIPCHK(h, kmpc_launch_probe<float>((const float *)a, (const float *)b, (float *)d, st));
    return KMPC_OK;
}

// ---- batched waypoint generation (scripts/gps_utils/ref_gps_traj.py) -------------------------------
struct kmpc_path {
    int device, M;
    double *d;  // t | X | Y | psi | s, each M doubles
    std::string err;
};

extern "C" int32_t kmpc_path_create(int32_t device, int32_t M, const double *t, const double *X, const double *Y,
                                    const double *psi, const double *cdist, kmpc_path **out)
{
    if (!out || M < 2 || !t || !X || !Y || !psi || !cdist) return fail(nullptr, KMPC_ERR_ARG, "kmpc_path_create: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, KMPC_ERR_NODEVICE, "kmpc_path_create: no HIP device");
    if (device < 0 || device >= ndev) return fail(nullptr, KMPC_ERR_ARG, "kmpc_path_create: device %d of %d", device, ndev);
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, KMPC_ERR_HIP, "kmpc_path_create: hipSetDevice failed");
    kmpc_path *p = new kmpc_path();
    p->device = device; p->M = M; p->d = nullptr;
    if (hipMalloc((void **)&p->d, (size_t)5 * M * sizeof(double)) != hipSuccess) { delete p; return fail(nullptr, KMPC_ERR_HIP, "kmpc_path_create: hipMalloc failed"); }
    const double *src[5] = {t, X, Y, psi, cdist};
    for (int i = 0; i < 5; ++i)
        if (hipMemcpy(p->d + (size_t)i * M, src[i], (size_t)M * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(p->d); delete p;
            return fail(nullptr, KMPC_ERR_HIP, "kmpc_path_create: hipMemcpy failed");
        }
    *out = p;
    return KMPC_OK;
}

extern "C" int32_t kmpc_path_destroy(kmpc_path *p)
{
    if (!p) return KMPC_OK;
    (void)hipSetDevice(p->device);
    (void)hipFree(p->d);
    delete p;
    return KMPC_OK;
}

extern "C" int32_t kmpc_waypoints_batch(kmpc_path *p, int32_t B, int32_t horizon, double traj_dt, const double *pose,
                                        const double *v_target, double *ref_out, int32_t *stop_out, int32_t *closest_out,
                                        void *stream)
{
    if (!p) return KMPC_ERR_ARG;
    if (B < 0 || horizon < 1 || horizon > 63 || !(traj_dt > 0)) { p->err = "kmpc_waypoints_batch: bad B / horizon / traj_dt"; return KMPC_ERR_ARG; }
    if (B == 0) return KMPC_OK;
    if (!pose || !ref_out || !stop_out) { p->err = "kmpc_waypoints_batch: null required buffer"; return KMPC_ERR_ARG; }
    if (hipSetDevice(p->device) != hipSuccess) { p->err = "hipSetDevice failed"; return KMPC_ERR_HIP; }
    WP w;
    w.M = p->M; w.B = B; w.H = horizon; w.use_vtarget = v_target ? 1 : 0; w.traj_dt = traj_dt;
    w.t = p->d; w.X = p->d + p->M; w.Y = p->d + 2 * (size_t)p->M; w.psi = p->d + 3 * (size_t)p->M; w.s = p->d + 4 * (size_t)p->M;
    w.pose = pose; w.vt = v_target; w.ref = ref_out; w.stop = stop_out; w.closest = closest_out;
    hipError_t e = kmpc_launch_waypoints(w, (hipStream_t)stream);
    if (e != hipSuccess) { p->err = std::string("waypoints launch failed: ") + hipGetErrorString(e); return KMPC_ERR_HIP; }
    return KMPC_OK;
}

extern "C" const char *kmpc_path_last_error(kmpc_path *p) { return p ? p->err.c_str() : g_create_err.c_str(); }

// ---- a set of recorded paths and a fleet that mixes them (kmpc_waypoints_fleet_kernel) ------------------------------
struct kmpc_pathset {
    int device, P, total;
    double *d;      // one allocation: t | X | Y | psi | s, each `total` doubles with the paths concatenated, then off[P+1] int32
    int32_t *off;   // points into d's allocation
    std::string err;
};

extern "C" int32_t kmpc_pathset_create(int32_t device, int32_t P, const int32_t *M, const double *t, const double *X, const double *Y,
                                       const double *psi, const double *cdist, kmpc_pathset **out)
{
    if (!out || P < 1 || !M || !t || !X || !Y || !psi || !cdist) return fail(nullptr, KMPC_ERR_ARG, "kmpc_pathset_create: bad argument");
    std::vector<int32_t> off((size_t)P + 1, 0);
    int64_t sum = 0;
    for (int p = 0; p < P; ++p) {
        if (M[p] < 2) return fail(nullptr, KMPC_ERR_ARG, "kmpc_pathset_create: path %d has %d samples (at least 2)", p, M[p]);
        sum += M[p];
        if (sum > INT32_MAX) return fail(nullptr, KMPC_ERR_ARG, "kmpc_pathset_create: more than 2^31 - 1 samples in all");
        off[p + 1] = (int32_t)sum;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, KMPC_ERR_NODEVICE, "kmpc_pathset_create: no HIP device");
    if (device < 0 || device >= ndev) return fail(nullptr, KMPC_ERR_ARG, "kmpc_pathset_create: device %d of %d", device, ndev);
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, KMPC_ERR_HIP, "kmpc_pathset_create: hipSetDevice failed");
    kmpc_pathset *ps = new kmpc_pathset();
    const size_t n = (size_t)sum;
    ps->device = device; ps->P = P; ps->total = (int)sum; ps->d = nullptr;
    if (hipMalloc((void **)&ps->d, 5 * n * sizeof(double) + off.size() * sizeof(int32_t)) != hipSuccess) {
        delete ps;
        return fail(nullptr, KMPC_ERR_HIP, "kmpc_pathset_create: hipMalloc failed");
    }
    ps->off = (int32_t *)(ps->d + 5 * n);
    const double *src[5] = {t, X, Y, psi, cdist};
    bool ok = hipMemcpy(ps->off, off.data(), off.size() * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess;
    for (int i = 0; i < 5 && ok; ++i) ok = hipMemcpy(ps->d + i * n, src[i], n * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        (void)hipFree(ps->d); delete ps;
        return fail(nullptr, KMPC_ERR_HIP, "kmpc_pathset_create: hipMemcpy failed");
    }
    *out = ps;
    return KMPC_OK;
}

extern "C" int32_t kmpc_pathset_destroy(kmpc_pathset *ps)
{
    if (!ps) return KMPC_OK;
    (void)hipSetDevice(ps->device);
    (void)hipFree(ps->d);
    delete ps;
    return KMPC_OK;
}

extern "C" int32_t kmpc_waypoints_fleet(kmpc_pathset *ps, int32_t B, int32_t horizon, double traj_dt, const double *pose,
                                        const int32_t *path_id, const uint8_t *time_mode, const double *v_target,
                                        double *ref_out, int32_t *stop_out, int32_t *closest_out, void *stream)
{
    if (!ps) return KMPC_ERR_ARG;
    if (B < 0 || horizon < 1 || horizon > 63 || !(traj_dt > 0)) { ps->err = "kmpc_waypoints_fleet: bad B / horizon / traj_dt"; return KMPC_ERR_ARG; }
    if (time_mode && !v_target) { ps->err = "kmpc_waypoints_fleet: time_mode needs v_target"; return KMPC_ERR_ARG; }
    if (B == 0) return KMPC_OK;
    if (!pose || !path_id || !ref_out || !stop_out) { ps->err = "kmpc_waypoints_fleet: null required buffer"; return KMPC_ERR_ARG; }
    if (hipSetDevice(ps->device) != hipSuccess) { ps->err = "hipSetDevice failed"; return KMPC_ERR_HIP; }
    WPF w;
    w.P = ps->P; w.B = B; w.H = horizon; w.total = ps->total; w.all_time = v_target ? 0 : 1; w.traj_dt = traj_dt;
    w.d = ps->d; w.off = ps->off; w.path_id = path_id; w.time_mode = time_mode;
    w.pose = pose; w.vt = v_target; w.ref = ref_out; w.stop = stop_out; w.closest = closest_out;
    hipError_t e = kmpc_launch_waypoints_fleet(w, (hipStream_t)stream);
    if (e != hipSuccess) { ps->err = std::string("fleet waypoints launch failed: ") + hipGetErrorString(e); return KMPC_ERR_HIP; }
    return KMPC_OK;
}

extern "C" const char *kmpc_pathset_last_error(kmpc_pathset *ps) { return ps ? ps->err.c_str() : g_create_err.c_str(); }

// ---- what the device-indexed and path-handle entry points below share --------------------------------------------------
// Every one of them checks its arguments first (each check answers before the first HIP call), returns KMPC_OK where there is nothing to do, and
// ends in on_device(): select the device, launch, and turn a hipError_t into the entry point's own text.
template <typename Launch>
static int32_t on_device(const char *fn, int device, Launch launch)
{
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, KMPC_ERR_HIP, "%s: hipSetDevice(%d) failed", fn, device);
    const hipError_t e = launch();
    if (e != hipSuccess) return fail(nullptr, KMPC_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
    return KMPC_OK;
}

static bool pos(double a) { return a > 0.0 && a <= 1.7976931348623157e308; }       // finite and > 0
static bool nonneg(double a) { return a >= 0.0 && a <= 1.7976931348623157e308; }   // finite and >= 0

// how a refusal words a pointer argument
static const char *given(const void *p) { return p ? "given" : "NULL"; }

// "fn: null required buffer (a given, b NULL, ...)" unless every one of the first `n` of `bufs` is given (an entry point that shares its list with
// a neighbour of more buffers names only its own); KMPC_OK when they all are.  The text is put together only on the way out.
struct Buf { const char *name; const void *p; };
static int32_t need_buffers(const char *fn, std::initializer_list<Buf> bufs, size_t n = (size_t)-1)
{
    const Buf *end = bufs.begin() + (n < bufs.size() ? n : bufs.size());
    bool all = true;
    for (const Buf *b = bufs.begin(); b != end; ++b) all = all && b->p;
    if (all) return KMPC_OK;
    std::string list;
    for (const Buf *b = bufs.begin(); b != end; ++b) list += std::string(b == bufs.begin() ? "" : ", ") + b->name + " " + given(b->p);
    return fail(nullptr, KMPC_ERR_ARG, "%s: null required buffer (%s)", fn, list.c_str());
}

// a table of `n` host rows of `words` doubles: zeros, then the {index, value} words of `set` in every row (the row fillers: kmpc_*_default,
// kmpc_*_init).  `refusal` is the caller's own sentence for n < 0 or a NULL table with n > 0: a format that is handed fn, n and the word for `rows`
// and takes as many of them as it says.
struct Word { int index; double value; };
static int32_t fill_rows(const char *fn, double *rows, int32_t n, int words, std::initializer_list<Word> set,
                         const char *refusal = "%s: bad argument (B=%d)")
{
    if (n < 0 || (n > 0 && !rows)) return fail(nullptr, KMPC_ERR_ARG, refusal, fn, n, given(rows));
    for (size_t b = 0; b < (size_t)n; ++b) {
        double *r = rows + (size_t)words * b;
        for (int i = 0; i < words; ++i) r[i] = 0.0;
        for (const Word &w : set) r[w.index] = w.value;
    }
    return KMPC_OK;
}

// the plant calls' common arguments, in the order their refusals are documented: B / n_updates / state / cmd, then the plant rows, then the road rows
// (where the entry point has them).  The drive rows and the queue follow in the callers, and only then "B == 0 or n_updates == 0: nothing to do".
static int32_t sim_args(const char *fn, int32_t B, int32_t n_updates, const void *state, const void *cmd, const void *plant, const void *road,
                        bool need_road)
{
    if (B < 0 || n_updates < 0 || (B > 0 && (!state || !cmd))) return fail(nullptr, KMPC_ERR_ARG, "%s: bad argument (B=%d, n_updates=%d)", fn, B, n_updates);
    if (B > 0 && !plant) return fail(nullptr, KMPC_ERR_ARG, "%s: null plant rows", fn);
    if (need_road && B > 0 && !road) return fail(nullptr, KMPC_ERR_ARG, "%s: null road rows", fn);
    return KMPC_OK;
}

// the command ring of the queue, road and drive plants: checked whatever B is
static int32_t queue_args(const char *fn, int32_t depth, int64_t period, const void *cmd_queue)
{
    if (depth < 2 || period < 0 || !cmd_queue)
        return fail(nullptr, KMPC_ERR_ARG, "%s: bad queue (depth=%d, at least 2; period=%lld, at least 0; cmd_queue %s)", fn, depth, (long long)period,
                    given(cmd_queue));
    return KMPC_OK;
}

// the plant calls' argument block: what every kind or every kind with rows has; the road and drive entries add their own words
static PlantCall plant_call(int32_t B, int32_t n_updates, void *state, const void *cmd, const void *plant, const int32_t *cmd_delay, void *cmd_log,
                            int32_t depth, int64_t period)
{
    return {B, n_updates, (double *)state, (const double *)cmd, (const double *)plant, cmd_delay, (double *)cmd_log, depth, (long long)period,
            nullptr, nullptr, nullptr, nullptr, nullptr};
}

// ---- tracking errors and the running score record (kmpc_track_score.hip) ----------------------------------------------
extern "C" int32_t kmpc_track_score_init(double *score_host, int32_t B)
{
    return fill_rows("kmpc_track_score_init", score_host, B, KMPC_SCORE_WORDS, {{KMPC_SCORE_LATCH_INDEX, -1.0}});
}

// the checks both entry points share, before the handle is touched; 1 = nothing to do (B = 0)
static int track_score_args(const char *fn, const void *handle, int B, const double *state, int stride, const int32_t *path_id, bool fleet,
                            double settle_tol, const int32_t *status, const int32_t *iters, const double *cmd, const uint8_t *latch)
{
    if (!handle) return fail(nullptr, KMPC_ERR_ARG, "%s: null path handle", fn);
    if (B < 0 || stride < 3) return fail(nullptr, KMPC_ERR_ARG, "%s: bad B / state_stride (B=%d, state_stride=%d; state_stride >= 3)", fn, B, stride);
    if (!std::isfinite(settle_tol) || settle_tol < 0) return fail(nullptr, KMPC_ERR_ARG, "%s: settle_tol must be finite and >= 0", fn);
    const int given = (status != nullptr) + (iters != nullptr) + (cmd != nullptr) + (latch != nullptr);
    if (given != 0 && given != 4) return fail(nullptr, KMPC_ERR_ARG, "%s: status, iters, cmd and stop_latch are given all together or all NULL", fn);
    if (B > 0 && (!state || (fleet && !path_id))) return fail(nullptr, KMPC_ERR_ARG, "%s: null required buffer", fn);
    return B == 0 ? 1 : KMPC_OK;
}

extern "C" int32_t kmpc_track_score_batch(kmpc_path *p, int32_t B, const double *state, int32_t state_stride, double settle_tol,
                                          const int32_t *status, const int32_t *iters, const double *cmd, const uint8_t *stop_latch,
                                          double *err_out, int32_t *seg_out, int32_t *closest_out, double *score, void *stream)
{
    const int rc = track_score_args("kmpc_track_score_batch", p, B, state, state_stride, nullptr, false, settle_tol, status, iters, cmd, stop_latch);
    if (rc != KMPC_OK) return rc < 0 ? rc : KMPC_OK;
    TSB k;
    k.w = {B, state_stride, settle_tol, state, status, iters, cmd, stop_latch, err_out, seg_out, closest_out, score};
    k.M = p->M; k.X = p->d + p->M; k.Y = p->d + 2 * (size_t)p->M; k.psi = p->d + 3 * (size_t)p->M; k.s = p->d + 4 * (size_t)p->M;
    return on_device("kmpc_track_score_batch", p->device, [&] { return kmpc_launch_track_score(k, (hipStream_t)stream); });
}

extern "C" int32_t kmpc_track_score_fleet(kmpc_pathset *ps, int32_t B, const double *state, int32_t state_stride, const int32_t *path_id,
                                          double settle_tol, const int32_t *status, const int32_t *iters, const double *cmd,
                                          const uint8_t *stop_latch, double *err_out, int32_t *seg_out, int32_t *closest_out, double *score,
                                          void *stream)
{
    const int rc = track_score_args("kmpc_track_score_fleet", ps, B, state, state_stride, path_id, true, settle_tol, status, iters, cmd, stop_latch);
    if (rc != KMPC_OK) return rc < 0 ? rc : KMPC_OK;
    TSF k;
    k.w = {B, state_stride, settle_tol, state, status, iters, cmd, stop_latch, err_out, seg_out, closest_out, score};
    k.P = ps->P; k.total = ps->total; k.d = ps->d; k.off = ps->off; k.path_id = path_id;
    return on_device("kmpc_track_score_fleet", ps->device, [&] { return kmpc_launch_track_score_fleet(k, (hipStream_t)stream); });
}

// ---- curvature table and speed plan (kmpc_speed_plan.hip) ------------------------------------------------------------
extern "C" int32_t kmpc_pathset_curvature(kmpc_pathset *ps, double window, double *kappa_out, void *stream)
{
    if (!ps) return fail(nullptr, KMPC_ERR_ARG, "kmpc_pathset_curvature: null path set");
    if (!std::isfinite(window) || !(window > 0)) return fail(nullptr, KMPC_ERR_ARG, "kmpc_pathset_curvature: window must be finite and > 0");
    if (!kappa_out) return fail(nullptr, KMPC_ERR_ARG, "kmpc_pathset_curvature: null kappa_out");
    const SPC k = {ps->P, ps->total, 0.5 * window, ps->d, ps->off, kappa_out};
    return on_device("kmpc_pathset_curvature", ps->device, [&] { return kmpc_launch_curvature(k, (hipStream_t)stream); });
}

// this project's own defaults (the reference has no such stage): the one place they exist
extern "C" int32_t kmpc_speed_plan_default(double *rows_host, int32_t B)
{
    return fill_rows("kmpc_speed_plan_default", rows_host, B, KMPC_PLAN_WORDS,
                     {{KMPC_PLAN_A_LAT, 2.0}, {KMPC_PLAN_A_BRAKE, 0.7}, {KMPC_PLAN_V_FLOOR, 1.0}, {KMPC_PLAN_END_STOP, 0.0}});
}

// both plan entry points: `profile` is the map of kmpc_speed_plan_fleet_profile (required there), null for kmpc_speed_plan_fleet
static int32_t speed_plan_fleet(const char *fn, bool with_profile, kmpc_pathset *ps, int32_t B, const double *kappa, const double *profile,
                                const double *state, int32_t state_stride, const int32_t *path_id, const double *v_cap, const double *rows,
                                double *v_plan_out, double *info_out, int32_t *closest_out, void *stream)
{
    if (!ps) return fail(nullptr, KMPC_ERR_ARG, "%s: null path set", fn);
    if (B < 0 || state_stride < 2)
        return fail(nullptr, KMPC_ERR_ARG, "%s: bad B / state_stride (B=%d, state_stride=%d; state_stride >= 2)", fn, B, state_stride);
    if (B > 0 && (!kappa || (with_profile && !profile) || !state || !path_id || !v_cap || !rows || !v_plan_out))
        return fail(nullptr, KMPC_ERR_ARG, "%s: null required buffer", fn);
    if (B == 0) return KMPC_OK;
    const SPF w = {ps->P, B, ps->total, state_stride, ps->d, ps->off, kappa, with_profile ? profile : nullptr, state, path_id, v_cap, rows,
                   v_plan_out, info_out, closest_out};
    return on_device(fn, ps->device, [&] { return kmpc_launch_speed_plan_fleet(w, (hipStream_t)stream); });
}

extern "C" int32_t kmpc_speed_plan_fleet(kmpc_pathset *ps, int32_t B, const double *kappa, const double *state, int32_t state_stride,
                                         const int32_t *path_id, const double *v_cap, const double *rows, double *v_plan_out, double *info_out,
                                         int32_t *closest_out, void *stream)
{
    return speed_plan_fleet("kmpc_speed_plan_fleet", false, ps, B, kappa, nullptr, state, state_stride, path_id, v_cap, rows, v_plan_out, info_out,
                            closest_out, stream);
}

extern "C" int32_t kmpc_speed_plan_fleet_profile(kmpc_pathset *ps, int32_t B, const double *kappa, const double *profile, const double *state,
                                                 int32_t state_stride, const int32_t *path_id, const double *v_cap, const double *rows,
                                                 double *v_plan_out, double *info_out, int32_t *closest_out, void *stream)
{
    return speed_plan_fleet("kmpc_speed_plan_fleet_profile", true, ps, B, kappa, profile, state, state_stride, path_id, v_cap, rows, v_plan_out,
                            info_out, closest_out, stream);
}

// ---- car following (kmpc_follow.hip; include/kmpc_follow.h) --------------------------------------------------------------
// this project's own defaults (the reference has no such stage): the one place they exist
extern "C" int32_t kmpc_follow_default(double *rows_host, int32_t B)
{
    return fill_rows("kmpc_follow_default", rows_host, B, KMPC_FOLLOW_WORDS,
                     {{KMPC_FOLLOW_D_MIN, 5.0}, {KMPC_FOLLOW_T_HEADWAY, 1.0}, {KMPC_FOLLOW_A_BRAKE, 0.7}, {KMPC_FOLLOW_K_GAP, 0.5}, {KMPC_FOLLOW_LENGTH, 4.9}});
}

extern "C" int32_t kmpc_follow_stat_init(double *stat_host, int32_t B)
{
    return fill_rows("kmpc_follow_stat_init", stat_host, B, KMPC_FOLLOWSTAT_WORDS, {{KMPC_FOLLOWSTAT_MIN_GAP, INFINITY}});
}

// the argument block of both follow entry points, checked in the documented order.  `order` is kmpc_order_follow_fleet's one more required buffer
// (`ordered`); kmpc_follow_fleet has none and does not name it.  1 = nothing to do (B = 0)
static int follow_args(const char *fn, const FL &w, const int32_t *order, bool ordered)
{
    if (w.B < 0 || w.s_stride < 1 || w.speed_stride < 1)
        return fail(nullptr, KMPC_ERR_ARG, "%s: bad B / s_stride / speed_stride (B=%d, s_stride=%d, speed_stride=%d; strides >= 1)", fn, w.B, w.s_stride,
                    w.speed_stride);
    if (w.B > 0 && need_buffers(fn, {{"s_along", w.s_along}, {"speed", w.speed}, {"rows", w.rows}, {"v_cap", w.v_cap}, {"v_cap_out", w.v_cap_out},
                                     {"order", order}}, ordered ? 6 : 5) != KMPC_OK)
        return KMPC_ERR_ARG;
    return w.B == 0 ? 1 : KMPC_OK;
}

extern "C" int32_t kmpc_follow_fleet(int32_t device, int32_t B, const double *s_along, int32_t s_stride, const double *speed, int32_t speed_stride,
                                     const int32_t *path_id, const uint8_t *present, const double *rows, const double *v_cap, double *v_cap_out,
                                     double *gap_out, int32_t *leader_out, double *stat, void *stream)
{
    const FL w = {B, s_stride, speed_stride, s_along, speed, path_id, present, rows, v_cap, v_cap_out, gap_out, leader_out, stat};
    const int rc = follow_args("kmpc_follow_fleet", w, nullptr, false);
    if (rc != KMPC_OK) return rc < 0 ? rc : KMPC_OK;
    return on_device("kmpc_follow_fleet", device, [&] { return kmpc_launch_follow_fleet(w, (hipStream_t)stream); });
}

// ---- lanes (kmpc_lanes.hip; include/kmpc_lanes.h) ---------------------------------------------------------------------------
// this project's own defaults (the reference has no such stage): the one place they exist
extern "C" int32_t kmpc_lane_default(double *rows_host, int32_t B)
{
    return fill_rows("kmpc_lane_default", rows_host, B, KMPC_LANE_WORDS,
                     {{KMPC_LANE_N_LANES, 1.0}, {KMPC_LANE_WIDTH, 3.5}, {KMPC_LANE_V_LAT, 1.0}, {KMPC_LANE_GAIN, 0.5}, {KMPC_LANE_HOLD, 20.0},
                      {KMPC_LANE_CLEAR_TOL, 0.5}, {KMPC_LANE_KEEP_RIGHT, 1.0}});
}

extern "C" int32_t kmpc_lane_rec_init(double *rec_host, int32_t B)
{
    return fill_rows("kmpc_lane_rec_init", rec_host, B, KMPC_LANEREC_WORDS, {{KMPC_LANEREC_MIN_GAP, INFINITY}});
}

// the argument block of both lane entry points, checked in the documented order, in two halves: between them kmpc_order_lane_step_fleet checks
// its own lanes_max and workspace size.  First B, k, the strides and dt ...
static int lane_scalars(const char *fn, const LN &w)
{
    if (w.B < 0 || w.k < 0 || w.s_stride < 1 || w.e_stride < 1 || w.speed_stride < 1)
        return fail(nullptr, KMPC_ERR_ARG, "%s: bad B / k / stride (B=%d, k=%d, s_stride=%d, e_stride=%d, speed_stride=%d; strides >= 1)", fn, w.B, w.k,
                    w.s_stride, w.e_stride, w.speed_stride);
    if (!pos(w.dt)) return fail(nullptr, KMPC_ERR_ARG, "%s: dt must be finite and > 0", fn);
    return KMPC_OK;
}

// ... then the buffers: `order` and `workspace` are the ordered entry point's two more required ones (`ordered`); kmpc_lane_step_fleet has
// neither and does not name them.  1 = nothing to do (B = 0)
static int lane_buffers(const char *fn, const LN &w, const int32_t *order, const void *workspace, bool ordered)
{
    if (w.B > 0 && need_buffers(fn, {{"s_along", w.s_along}, {"e_ct", w.e_ct}, {"speed", w.speed}, {"follow_rows", w.follow_rows},
                                     {"lane_rows", w.lane_rows}, {"v_cap", w.v_cap}, {"v_cap_out", w.v_cap_out}, {"occ_in", w.occ_in},
                                     {"occ_out", w.occ_out}, {"rec", w.rec}, {"order", order}, {"workspace", workspace}}, ordered ? 12 : 10) != KMPC_OK)
        return KMPC_ERR_ARG;
    if (w.B > 0 && w.occ_in == w.occ_out)
        return fail(nullptr, KMPC_ERR_ARG, "%s: occ_in == occ_out (the occupancy every vehicle reads is a snapshot nobody writes)", fn);
    return w.B == 0 ? 1 : KMPC_OK;
}

extern "C" int32_t kmpc_lane_step_fleet(int32_t device, int32_t B, int32_t k, double dt, const double *s_along, int32_t s_stride, const double *e_ct,
                                        int32_t e_stride, const double *speed, int32_t speed_stride, const int32_t *path_id,
                                        const uint8_t *present, const double *follow_rows, const double *lane_rows, const double *v_cap,
                                        double *v_cap_out, const uint32_t *occ_in, uint32_t *occ_out, double *rec, double *gap_out,
                                        int32_t *leader_out, double *nbr_out, void *stream)
{
    const LN w = {B, k, s_stride, e_stride, speed_stride, dt, s_along, e_ct, speed, path_id, present, follow_rows, lane_rows, v_cap, v_cap_out,
                  occ_in, occ_out, rec, gap_out, leader_out, nbr_out};
    int rc = lane_scalars("kmpc_lane_step_fleet", w);
    if (rc == KMPC_OK) rc = lane_buffers("kmpc_lane_step_fleet", w, nullptr, nullptr, false);
    if (rc != KMPC_OK) return rc < 0 ? rc : KMPC_OK;
    return on_device("kmpc_lane_step_fleet", device, [&] { return kmpc_launch_lane_step(w, (hipStream_t)stream); });
}

extern "C" int32_t kmpc_ref_offset_batch(int32_t device, int32_t B, int32_t H1, double *ref, const double *offset, int32_t offset_stride, void *stream)
{
    if (B < 0 || H1 < 1 || offset_stride < 1 || (long long)B * H1 > 2147483647LL)
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_ref_offset_batch: bad B / H1 / offset_stride (B=%d, H1=%d, >= 1, B * H1 < 2^31; offset_stride=%d, >= 1)",
                    B, H1, offset_stride);
    if (B > 0 && need_buffers("kmpc_ref_offset_batch", {{"ref", ref}, {"offset", offset}}) != KMPC_OK) return KMPC_ERR_ARG;
    if (B == 0) return KMPC_OK;
    const RO w = {B, H1, offset_stride, ref, offset};
    return on_device("kmpc_ref_offset_batch", device, [&] { return kmpc_launch_ref_offset(w, (hipStream_t)stream); });
}

// ---- range sensor and leader tracker (kmpc_range.hip; include/kmpc_range.h) -------------------------------------------------
// this project's own defaults (the reference has no such stage): the one place they exist
extern "C" int32_t kmpc_range_default(double *rows_host, int32_t B)
{
    return fill_rows("kmpc_range_default", rows_host, B, KMPC_RANGE_WORDS,
                     {{KMPC_RANGE_RANGE_MAX, 120.0}, {KMPC_RANGE_SIGMA_R, 0.25}, {KMPC_RANGE_SIGMA_V, 0.12}, {KMPC_RANGE_FILTER, 1.0},
                      {KMPC_RANGE_COAST_MAX, 5.0}, {KMPC_RANGE_Q_GAP, 0.01}, {KMPC_RANGE_Q_V, 0.25}, {KMPC_RANGE_R_GAP, 0.0625}, {KMPC_RANGE_R_V, 0.0144}});
}

extern "C" int32_t kmpc_range_rec_init(double *rec_host, int32_t B)
{
    return fill_rows("kmpc_range_rec_init", rec_host, B, KMPC_RANGEREC_WORDS, {{KMPC_RANGEREC_TRACK_ID, -1.0}});
}

extern "C" int32_t kmpc_range_follow_batch(int32_t device, int32_t B, double dt, const double *truth, const int32_t *leader, const double *speed_true,
                                           int32_t speed_true_stride, const double *speed_known, int32_t speed_known_stride,
                                           const double *follow_rows, const double *range_rows, uint64_t seed, int64_t period, int64_t id_base,
                                           const double *v_cap, double *v_cap_out, double *rec, double *meas_out, void *stream)
{
    if (B < 0 || speed_true_stride < 1 || speed_known_stride < 1)
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_range_follow_batch: bad B / stride (B=%d, speed_true_stride=%d, speed_known_stride=%d; strides >= 1)", B,
                    speed_true_stride, speed_known_stride);
    if (!pos(dt)) return fail(nullptr, KMPC_ERR_ARG, "kmpc_range_follow_batch: dt must be finite and > 0");
    if (period < 0 || period >= ((int64_t)1 << 61))
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_range_follow_batch: bad period (%lld; 0 <= period < 2^61)", (long long)period);
    if (B > 0 && need_buffers("kmpc_range_follow_batch", {{"truth", truth}, {"leader", leader}, {"speed_true", speed_true}, {"speed_known", speed_known},
                                                          {"follow_rows", follow_rows}, {"range_rows", range_rows}, {"v_cap", v_cap},
                                                          {"v_cap_out", v_cap_out}, {"rec", rec}}) != KMPC_OK)
        return KMPC_ERR_ARG;
    if (B == 0) return KMPC_OK;
    const RG w = {B, speed_true_stride, speed_known_stride, dt, seed, (uint64_t)period, (uint64_t)id_base, truth, leader, speed_true, speed_known,
                  follow_rows, range_rows, v_cap, v_cap_out, rec, meas_out};
    return on_device("kmpc_range_follow_batch", device, [&] { return kmpc_launch_range_follow(w, (hipStream_t)stream); });
}

// ---- the order of a fleet and the searches along it (kmpc_order.hip; include/kmpc_order.h) ----------------------------------
extern "C" int32_t kmpc_order_bytes(int32_t B, int32_t lanes_max, int64_t *bytes_out)
{
    if (B < 0 || lanes_max < 0 || lanes_max > 32 || !bytes_out)
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_order_bytes: bad argument (B=%d, lanes_max=%d (0 ... 32), bytes_out %s)", B, lanes_max,
                    given(bytes_out));
    *bytes_out = (int64_t)kmpc_order_layout(B, lanes_max).bytes;
    return KMPC_OK;
}

extern "C" int32_t kmpc_order_fleet(int32_t device, int32_t B, const double *s_along, int32_t s_stride, const double *speed, int32_t speed_stride,
                                    const int32_t *path_id, const uint8_t *present, int32_t *order_out, int32_t *count_out, void *workspace,
                                    int64_t workspace_bytes, void *stream)
{
    if (B < 0 || s_stride < 1 || speed_stride < 1)
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_order_fleet: bad B / s_stride / speed_stride (B=%d, s_stride=%d, speed_stride=%d; strides >= 1)", B,
                    s_stride, speed_stride);
    const OrderLayout o = kmpc_order_layout(B, 0);
    if (workspace_bytes < (int64_t)o.bytes)
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_order_fleet: workspace_bytes %lld < kmpc_order_bytes(%d, 0) = %lld", (long long)workspace_bytes, B,
                    (long long)o.bytes);
    if (B > 0 && need_buffers("kmpc_order_fleet", {{"s_along", s_along}, {"speed", speed}, {"order_out", order_out}, {"workspace", workspace}}) != KMPC_OK)
        return KMPC_ERR_ARG;
    if (B == 0) return KMPC_OK;
    char *ws = (char *)workspace;
    const OS w = {B, s_stride, speed_stride, s_along, speed, path_id, present, order_out, count_out, (uint64_t *)(ws + o.key_lo),
                  (uint32_t *)(ws + o.key_hi), (int32_t *)(ws + o.idx), (uint32_t *)(ws + o.hist), (uint64_t *)(ws + o.blk),
                  (uint32_t *)(ws + o.flags), o.key_blocks, o.sort_blocks, o.chunk};
    return on_device("kmpc_order_fleet", device, [&] { return kmpc_launch_order(w, (hipStream_t)stream); });
}

extern "C" int32_t kmpc_order_follow_fleet(int32_t device, int32_t B, const double *s_along, int32_t s_stride, const double *speed,
                                           int32_t speed_stride, const int32_t *path_id, const uint8_t *present, const double *rows,
                                           const double *v_cap, double *v_cap_out, double *gap_out, int32_t *leader_out, double *stat,
                                           const int32_t *order, void *stream)
{
    const OF w = {{B, s_stride, speed_stride, s_along, speed, path_id, present, rows, v_cap, v_cap_out, gap_out, leader_out, stat}, order};
    const int rc = follow_args("kmpc_order_follow_fleet", w.f, order, true);
    if (rc != KMPC_OK) return rc < 0 ? rc : KMPC_OK;
    return on_device("kmpc_order_follow_fleet", device, [&] { return kmpc_launch_order_follow(w, (hipStream_t)stream); });
}

extern "C" int32_t kmpc_order_lane_step_fleet(int32_t device, int32_t B, int32_t k, double dt, const double *s_along, int32_t s_stride,
                                              const double *e_ct, int32_t e_stride, const double *speed, int32_t speed_stride,
                                              const int32_t *path_id, const uint8_t *present, const double *follow_rows, const double *lane_rows,
                                              const double *v_cap, double *v_cap_out, const uint32_t *occ_in, uint32_t *occ_out, double *rec,
                                              double *gap_out, int32_t *leader_out, double *nbr_out, const int32_t *order, int32_t lanes_max,
                                              void *workspace, int64_t workspace_bytes, void *stream)
{
    const LN l = {B, k, s_stride, e_stride, speed_stride, dt, s_along, e_ct, speed, path_id, present, follow_rows, lane_rows, v_cap, v_cap_out,
                  occ_in, occ_out, rec, gap_out, leader_out, nbr_out};
    int rc = lane_scalars("kmpc_order_lane_step_fleet", l);
    if (rc != KMPC_OK) return rc;
    if (lanes_max < 0 || lanes_max > 32) return fail(nullptr, KMPC_ERR_ARG, "kmpc_order_lane_step_fleet: lanes_max %d outside 0 ... 32", lanes_max);
    const OrderLayout o = kmpc_order_layout(B, lanes_max);
    if (workspace_bytes < (int64_t)o.bytes)
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_order_lane_step_fleet: workspace_bytes %lld < kmpc_order_bytes(%d, %d) = %lld",
                    (long long)workspace_bytes, B, lanes_max, (long long)o.bytes);
    rc = lane_buffers("kmpc_order_lane_step_fleet", l, order, workspace, true);
    if (rc != KMPC_OK) return rc < 0 ? rc : KMPC_OK;
    char *ws = (char *)workspace;
    const OL w = {l, order, lanes_max, o.lane_blocks, (int32_t *)(ws + o.nxt), (int32_t *)(ws + o.prv), (int32_t *)(ws + o.first),
                  (int32_t *)(ws + o.last), (int32_t *)(ws + o.carry_next), (int32_t *)(ws + o.carry_prev)};
    return on_device("kmpc_order_lane_step_fleet", device, [&] { return kmpc_launch_order_lane_step(w, (hipStream_t)stream); });
}

// ---- road profile per path sample (kmpc_road_profile.hip) ----------------------------------------------------------------
extern "C" int32_t kmpc_road_profile_default(double *rows_host, int32_t n)
{
    return fill_rows("kmpc_road_profile_default", rows_host, n, KMPC_PROFILE_WORDS, {{KMPC_PROFILE_MU_SCALE, 1.0}, {KMPC_PROFILE_V_LIMIT, INFINITY}},
                     "%s: bad argument (n=%d)");
}

extern "C" int32_t kmpc_road_profile_fleet(kmpc_pathset *ps, int32_t B, const double *profile, const double *state, int32_t state_stride,
                                           const int32_t *path_id, const double *road_base, double *road_out, int32_t *closest_out, void *stream)
{
    if (!ps) return fail(nullptr, KMPC_ERR_ARG, "kmpc_road_profile_fleet: null path set");
    if (B < 0 || state_stride < 2)
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_road_profile_fleet: bad B / state_stride (B=%d, state_stride=%d; state_stride >= 2)", B, state_stride);
    if (B > 0 && (!profile || !state || !path_id || !road_base || !road_out))
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_road_profile_fleet: null required buffer");
    if (road_out && road_out == road_base)
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_road_profile_fleet: road_out must not be road_base (the scaling would compound call after call)");
    if (B == 0) return KMPC_OK;
    const RPF w = {ps->P, B, ps->total, state_stride, ps->d, ps->off, profile, state, path_id, road_base, road_out, closest_out};
    return on_device("kmpc_road_profile_fleet", ps->device, [&] { return kmpc_launch_road_profile_fleet(w, (hipStream_t)stream); });
}

// ---- closed-loop simulator (kmpc_sim.hip) ------------------------------------------------------------------------
extern "C" int32_t kmpc_sim_advance_batch(int32_t device, int32_t B, void *state, const void *cmd, int32_t n_updates, void *stream)
{
    if (B < 0 || n_updates < 0 || (B > 0 && (!state || !cmd))) return fail(nullptr, KMPC_ERR_ARG, "kmpc_sim_advance_batch: bad argument (B=%d, n_updates=%d)", B, n_updates);
    if (B == 0 || n_updates == 0) return KMPC_OK;
    const PlantCall k = plant_call(B, n_updates, state, cmd, nullptr, nullptr, nullptr, 0, 0);
    return on_device("kmpc_sim_advance_batch", device, [&] { return kmpc_launch_plant(KMPC_PLANT_FIXED, k, (hipStream_t)stream); });
}

// the reference's plant constants (vehicle_simulator.py:61-67, :112-113): the one place they exist for the per-vehicle plant
extern "C" int32_t kmpc_plant_default(double *row8)
{
    if (!row8) return fail(nullptr, KMPC_ERR_ARG, "kmpc_plant_default: null row");
    row8[KMPC_PLANT_LF] = 1.152; row8[KMPC_PLANT_LR] = 1.693; row8[KMPC_PLANT_M] = 1840.0; row8[KMPC_PLANT_IZ] = 3477.0;
    row8[KMPC_PLANT_C_ALPHA_F] = 4.0703e4; row8[KMPC_PLANT_C_ALPHA_R] = 6.4495e4; row8[KMPC_PLANT_K_ACC] = 5.0; row8[KMPC_PLANT_K_DF] = 5.0;
    return KMPC_OK;
}

extern "C" int32_t kmpc_sim_advance_plant(int32_t device, int32_t B, void *state, const void *cmd, const void *plant, const int32_t *cmd_delay,
                                          void *cmd_held, int32_t n_updates, void *stream)
{
    int32_t rc = sim_args("kmpc_sim_advance_plant", B, n_updates, state, cmd, plant, nullptr, false);
    if (rc != KMPC_OK) return rc;
    if (B > 0 && cmd_delay && !cmd_held) return fail(nullptr, KMPC_ERR_ARG, "kmpc_sim_advance_plant: cmd_delay needs cmd_held");
    if (B == 0 || n_updates == 0) return KMPC_OK;
    const PlantCall k = plant_call(B, n_updates, state, cmd, plant, cmd_delay, cmd_held, 0, 0);
    return on_device("kmpc_sim_advance_plant", device, [&] { return kmpc_launch_plant(KMPC_PLANT_ROWS, k, (hipStream_t)stream); });
}

extern "C" int32_t kmpc_sense_batch(int32_t device, int32_t B, const void *state, const void *sensor, uint64_t seed, int64_t period, int64_t id_base,
                                    void *est, void *stream)
{
    if (B < 0 || period < 0 || id_base < 0 || (B > 0 && (!state || !sensor || !est)))
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_sense_batch: bad argument (B=%d, period=%lld, id_base=%lld)", B, (long long)period, (long long)id_base);
    if (B == 0) return KMPC_OK;
    return on_device("kmpc_sense_batch", device, [&] {
        return kmpc_launch_sense(B, (const double *)state, (const double *)sensor, seed, (uint64_t)period, (uint64_t)id_base, nullptr, nullptr, 0, (double *)est,
                                 (hipStream_t)stream);
    });
}

extern "C" int32_t kmpc_sim_advance_queue(int32_t device, int32_t B, void *state, const void *cmd, const void *plant, const int32_t *cmd_delay,
                                          void *cmd_queue, int32_t depth, int64_t period, int32_t n_updates, void *stream)
{
    int32_t rc = sim_args("kmpc_sim_advance_queue", B, n_updates, state, cmd, plant, nullptr, false);
    if (rc != KMPC_OK) return rc;
    if ((rc = queue_args("kmpc_sim_advance_queue", depth, period, cmd_queue)) != KMPC_OK) return rc;
    if (B == 0 || n_updates == 0) return KMPC_OK;
    const PlantCall k = plant_call(B, n_updates, state, cmd, plant, cmd_delay, cmd_queue, depth, period);
    return on_device("kmpc_sim_advance_queue", device, [&] { return kmpc_launch_plant(KMPC_PLANT_QUEUE, k, (hipStream_t)stream); });
}

// the neutral road row: no grip limit, a flat and level road, no steering offset, the acceleration as commanded
extern "C" int32_t kmpc_road_default(double *row8)
{
    if (!row8) return fail(nullptr, KMPC_ERR_ARG, "kmpc_road_default: null row");
    row8[KMPC_ROAD_MU_F] = INFINITY; row8[KMPC_ROAD_MU_R] = INFINITY; row8[KMPC_ROAD_A_LONG] = 0.0; row8[KMPC_ROAD_A_LAT] = 0.0;
    row8[KMPC_ROAD_DF_OFFSET] = 0.0; row8[KMPC_ROAD_ACC_GAIN] = 1.0; row8[6] = 0.0; row8[7] = 0.0;
    return KMPC_OK;
}

extern "C" int32_t kmpc_sim_advance_road(int32_t device, int32_t B, void *state, const void *cmd, const void *plant, const void *road,
                                         const int32_t *cmd_delay, void *cmd_queue, int32_t depth, int64_t period, int32_t n_updates, void *road_stat,
                                         void *stream)
{
    int32_t rc = sim_args("kmpc_sim_advance_road", B, n_updates, state, cmd, plant, road, true);
    if (rc != KMPC_OK) return rc;
    if ((rc = queue_args("kmpc_sim_advance_road", depth, period, cmd_queue)) != KMPC_OK) return rc;
    if (B == 0 || n_updates == 0) return KMPC_OK;
    PlantCall k = plant_call(B, n_updates, state, cmd, plant, cmd_delay, cmd_queue, depth, period);
    k.road = (const double *)road; k.road_stat = (double *)road_stat;
    return on_device("kmpc_sim_advance_road", device, [&] { return kmpc_launch_plant(KMPC_PLANT_ROAD, k, (hipStream_t)stream); });
}

// ---- low-level controller and pedal-driven plant (kmpc_drive.hip) ----------------------------------------------------
// the reference node's constants (LowLevelController.cpp:49-72, .h:113-118; the mass at fuel level 0, as before the first fuel report)
extern "C" int32_t kmpc_llc_default(double *row8)
{
    if (!row8) return fail(nullptr, KMPC_ERR_ARG, "kmpc_llc_default: null row");
    row8[KMPC_LLC_KP] = 0.8; row8[KMPC_LLC_KI] = 0.4; row8[KMPC_LLC_ACCEL_MAX] = 1.0; row8[KMPC_LLC_DECEL_MAX] = 1.0;
    row8[KMPC_LLC_STEER_RATIO] = 14.8; row8[KMPC_LLC_MASS] = 1847.78; row8[KMPC_LLC_BRAKE_DEADBAND] = 0.1; row8[KMPC_LLC_WHEEL_RADIUS] = 0.33;
    return KMPC_OK;
}

// the powertrain's constants: this project's choice (the reference has no powertrain model)
extern "C" int32_t kmpc_drive_default(double *row8)
{
    if (!row8) return fail(nullptr, KMPC_ERR_ARG, "kmpc_drive_default: null row");
    row8[KMPC_DRIVE_F_PEAK] = 6000.0; row8[KMPC_DRIVE_P_MAX] = 120e3; row8[KMPC_DRIVE_K_TH] = 5.0; row8[KMPC_DRIVE_K_BR] = 5.0;
    row8[KMPC_DRIVE_C_ROLL] = 0.15; row8[KMPC_DRIVE_C_DRAG] = 4e-4; row8[KMPC_DRIVE_STEER_RATIO] = 14.8; row8[KMPC_DRIVE_WHEEL_RADIUS] = 0.33;
    return KMPC_OK;
}

extern "C" int32_t kmpc_llc_step_batch(int32_t device, int32_t B, const void *cmd, const void *speed, int32_t speed_stride, const void *llc,
                                       void *llc_rec, void *pedals_out, void *stream)
{
    if (B < 0 || speed_stride < 1 || (B > 0 && (!cmd || !speed || !llc || !llc_rec)))
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_llc_step_batch: bad argument (B=%d, speed_stride=%d, at least 1; cmd, speed, llc and llc_rec are required)", B,
                    speed_stride);
    if (B == 0) return KMPC_OK;
    return on_device("kmpc_llc_step_batch", device, [&] {
        return kmpc_launch_llc_step(B, (const double *)cmd, (const double *)speed, speed_stride, (const double *)llc, (double *)llc_rec, (double *)pedals_out,
                                    (hipStream_t)stream);
    });
}

extern "C" int32_t kmpc_sim_advance_drive(int32_t device, int32_t B, void *state, const void *cmd, const void *plant, const void *road,
                                          const void *drive, const void *llc, void *llc_rec, const int32_t *cmd_delay, void *cmd_queue, int32_t depth,
                                          int64_t period, int32_t n_updates, void *road_stat, void *stream)
{
    int32_t rc = sim_args("kmpc_sim_advance_drive", B, n_updates, state, cmd, plant, road, true);
    if (rc != KMPC_OK) return rc;
    if (B > 0 && (!drive || !llc || !llc_rec)) return fail(nullptr, KMPC_ERR_ARG, "kmpc_sim_advance_drive: null drive rows, llc rows or llc_rec");
    if ((rc = queue_args("kmpc_sim_advance_drive", depth, period, cmd_queue)) != KMPC_OK) return rc;
    if (B == 0 || n_updates == 0) return KMPC_OK;
    PlantCall k = plant_call(B, n_updates, state, cmd, plant, cmd_delay, cmd_queue, depth, period);
    k.road = (const double *)road; k.road_stat = (double *)road_stat;
    k.drive = (const double *)drive; k.llc_rows = (const double *)llc; k.llc_rec = (double *)llc_rec;
    return on_device("kmpc_sim_advance_drive", device, [&] { return kmpc_launch_plant(KMPC_PLANT_DRIVE, k, (hipStream_t)stream); });
}

extern "C" int32_t kmpc_sense_delayed_batch(int32_t device, int32_t B, const void *state, const void *sensor, uint64_t seed, int64_t period,
                                            int64_t id_base, const int32_t *meas_delay, void *truth_ring, int32_t depth, void *est, void *stream)
{
    if (B < 0 || period < 0 || id_base < 0 || (B > 0 && (!state || !sensor || !est)))
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_sense_delayed_batch: bad argument (B=%d, period=%lld, id_base=%lld)", B, (long long)period, (long long)id_base);
    if (depth < 1 || (B > 0 && (!meas_delay || !truth_ring)))
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_sense_delayed_batch: bad ring (depth=%d, at least 1; meas_delay and truth_ring are required)", depth);
    if (B == 0) return KMPC_OK;
    return on_device("kmpc_sense_delayed_batch", device, [&] {
        return kmpc_launch_sense(B, (const double *)state, (const double *)sensor, seed, (uint64_t)period, (uint64_t)id_base, meas_delay,
                                 (double *)truth_ring, depth, (double *)est, (hipStream_t)stream);
    });
}

// ---- measurement stage with sensor faults (kmpc_sense_faults.hip) ------------------------------------------------------
// the neutral fault row: no source is ever lost, a lost one returns at once, no window, no outlier, never blind
extern "C" int32_t kmpc_sense_faults_default(double *rows_host, int32_t B)
{
    return fill_rows("kmpc_sense_faults_default", rows_host, B, KMPC_FAULT_WORDS,
                     {{KMPC_FAULT_P_REGAIN_GPS, 1.0}, {KMPC_FAULT_P_REGAIN_IMU, 1.0}, {KMPC_FAULT_P_REGAIN_SPD, 1.0}, {KMPC_FAULT_MAX_AGE, INFINITY}},
                     "%s: bad argument (B=%d, rows %s)");
}

extern "C" int32_t kmpc_sense_faults_batch(int32_t device, int32_t B, const void *state, const void *sensor, const void *faults, uint64_t seed,
                                           int64_t period, int64_t id_base, const int32_t *meas_delay, void *truth_ring, int32_t depth,
                                           void *fault_rec, void *z_out, void *held_out, int32_t *flags_out, uint8_t *blind_out, void *stream)
{
    if (B < 0 || period < 0 || id_base < 0 || (B > 0 && (!state || !sensor || !faults || !fault_rec || !z_out || !held_out)))
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_sense_faults_batch: bad argument (B=%d, period=%lld, id_base=%lld; state, sensor, faults, fault_rec, "
                    "z_out and held_out are required)", B, (long long)period, (long long)id_base);
    if ((meas_delay != nullptr) != (truth_ring != nullptr))
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_sense_faults_batch: meas_delay and truth_ring go together (meas_delay %s, truth_ring %s)",
                    given(meas_delay), given(truth_ring));
    if (meas_delay && depth < 1) return fail(nullptr, KMPC_ERR_ARG, "kmpc_sense_faults_batch: bad ring (depth=%d, at least 1)", depth);
    if (B == 0) return KMPC_OK;
    return on_device("kmpc_sense_faults_batch", device, [&] {
        return kmpc_launch_sense_faults(B, (const double *)state, (const double *)sensor, (const double *)faults, seed, (uint64_t)period, (uint64_t)id_base,
                                        meas_delay, (double *)truth_ring, depth, (double *)fault_rec, (double *)z_out, (double *)held_out, flags_out, blind_out,
                                        (hipStream_t)stream);
    });
}

// ---- Gauss-Markov stage (kmpc_wander.hip) ----------------------------------------------------------------------------
// the neutral row: 24 zeros, every channel off
extern "C" int32_t kmpc_wander_default(double *rows_host, int32_t B)
{
    return fill_rows("kmpc_wander_default", rows_host, B, KMPC_WANDER_WORDS, {}, "%s: bad argument (B=%d, rows %s)");
}

extern "C" int32_t kmpc_wander_batch(int32_t device, int32_t B, const void *wander, void *wander_rec, uint64_t seed, int64_t period, int64_t id_base,
                                     const void *sensor_base, void *sensor_out, const void *road_base, void *road_out, void *stream)
{
    if (B < 0 || period < 0 || id_base < 0 || period >= ((int64_t)1 << 62) || (B > 0 && (!wander || !wander_rec)))
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_wander_batch: bad argument (B=%d, period=%lld, below 2^62; id_base=%lld; wander %s, wander_rec %s)", B,
                    (long long)period, (long long)id_base, given(wander), given(wander_rec));
    if ((sensor_base != nullptr) != (sensor_out != nullptr) || (road_base != nullptr) != (road_out != nullptr))
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_wander_batch: a base and its out go together (sensor_base %s, sensor_out %s, road_base %s, road_out %s)",
                    given(sensor_base), given(sensor_out), given(road_base), given(road_out));
    if ((sensor_out && sensor_out == sensor_base) || (road_out && road_out == road_base))
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_wander_batch: an out must not be its base (the sum would compound call after call)");
    if (B == 0) return KMPC_OK;
    return on_device("kmpc_wander_batch", device, [&] {
        return kmpc_launch_wander(B, (const double *)wander, (double *)wander_rec, seed, (uint64_t)period, (uint64_t)id_base, (const double *)sensor_base,
                                  (double *)sensor_out, (const double *)road_base, (double *)road_out, (hipStream_t)stream);
    });
}

// ---- delay compensation (kmpc_latency.hip) ---------------------------------------------------------------------------
static int32_t latency_args(const char *fn, int32_t B, const void *cmd_hist, int32_t depth, int64_t period, int32_t n_updates, const int32_t *cmd_delay,
                            const int32_t *meas_delay, int32_t max_cmd_delay, int32_t max_meas_delay)
{
    if (B < 0 || period < 0 || n_updates < 1 || max_cmd_delay < 0 || max_meas_delay < 0)
        return fail(nullptr, KMPC_ERR_ARG, "%s: bad argument (B=%d, period=%lld, n_updates=%d, max_cmd_delay=%d, max_meas_delay=%d)", fn, B,
                    (long long)period, n_updates, max_cmd_delay, max_meas_delay);
    const int64_t need = (int64_t)max_meas_delay + ((int64_t)max_cmd_delay + n_updates - 1) / n_updates + 1;
    if ((int64_t)depth < need)
        return fail(nullptr, KMPC_ERR_ARG, "%s: depth=%d, but max_meas_delay=%d periods + max_cmd_delay=%d updates of %d per period reach back %lld periods",
                    fn, depth, max_meas_delay, max_cmd_delay, n_updates, (long long)need);
    if (B > 0 && (!cmd_hist || !cmd_delay || !meas_delay)) return fail(nullptr, KMPC_ERR_ARG, "%s: null required buffer", fn);
    return KMPC_OK;
}

extern "C" int32_t kmpc_cmd_in_force_batch(int32_t device, int32_t B, const void *cmd_hist, int32_t depth, int64_t period, int32_t n_updates,
                                           const int32_t *cmd_delay, const int32_t *meas_delay, int32_t max_cmd_delay, int32_t max_meas_delay,
                                           void *u_out, void *stream)
{
    const int32_t rc = latency_args("kmpc_cmd_in_force_batch", B, cmd_hist, depth, period, n_updates, cmd_delay, meas_delay, max_cmd_delay, max_meas_delay);
    if (rc != KMPC_OK) return rc;
    if (B > 0 && !u_out) return fail(nullptr, KMPC_ERR_ARG, "kmpc_cmd_in_force_batch: null u_out");
    if (B == 0) return KMPC_OK;
    return on_device("kmpc_cmd_in_force_batch", device, [&] {
        return kmpc_launch_cmd_in_force(B, (const double *)cmd_hist, depth, (long long)period, n_updates, cmd_delay, meas_delay, max_cmd_delay, max_meas_delay,
                                        (double *)u_out, (hipStream_t)stream);
    });
}

extern "C" int32_t kmpc_predict_ahead_batch(int32_t device, int32_t B, const void *z, const void *cmd_hist, int32_t depth, int64_t period,
                                            int32_t n_updates, const int32_t *cmd_delay, const int32_t *meas_delay, int32_t max_cmd_delay,
                                            int32_t max_meas_delay, double L_a, double L_b, void *z_out, void *stream)
{
    const int32_t rc = latency_args("kmpc_predict_ahead_batch", B, cmd_hist, depth, period, n_updates, cmd_delay, meas_delay, max_cmd_delay, max_meas_delay);
    if (rc != KMPC_OK) return rc;
    if (!pos(L_a) || !pos(L_b)) return fail(nullptr, KMPC_ERR_ARG, "kmpc_predict_ahead_batch: L_a=%g, L_b=%g must be finite and > 0", L_a, L_b);
    if (B > 0 && (!z || !z_out)) return fail(nullptr, KMPC_ERR_ARG, "kmpc_predict_ahead_batch: null z or z_out");
    if (B == 0) return KMPC_OK;
    return on_device("kmpc_predict_ahead_batch", device, [&] {
        return kmpc_launch_predict_ahead(B, (const double *)z, (const double *)cmd_hist, depth, (long long)period, n_updates, cmd_delay, meas_delay, max_cmd_delay,
                                         max_meas_delay, L_a, L_b, (double *)z_out, (hipStream_t)stream);
    });
}

// ---- state estimator (kmpc_estimator.hip) --------------------------------------------------------------------------
extern "C" int32_t kmpc_estimate_batch(int32_t device, int32_t B, void *rec, const void *z, const void *u, int32_t u_stride, const void *params,
                                       double dt, double L_a, double L_b, double gate, void *est_out, void *innov_out, int32_t *flags_out,
                                       void *stream)
{
    if (B < 0 || u_stride < 2 || !pos(dt) || !pos(L_a) || !pos(L_b) || !(gate == 0.0 || pos(gate)))
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_estimate_batch: bad argument (B=%d, u_stride=%d, dt=%g, L_a=%g, L_b=%g, gate=%g)", B, u_stride, dt, L_a,
                    L_b, gate);
    if (B > 0 && (!rec || !z || !u || !params || !est_out)) return fail(nullptr, KMPC_ERR_ARG, "kmpc_estimate_batch: null required buffer");
    if (B == 0) return KMPC_OK;
    return on_device("kmpc_estimate_batch", device, [&] {
        return kmpc_launch_estimate(B, (double *)rec, (const double *)z, (const double *)u, u_stride, (const double *)params, dt, L_a, L_b, gate, (double *)est_out,
                                    (double *)innov_out, flags_out, (hipStream_t)stream);
    });
}

// ---- disturbance observer and command offset (kmpc_observer.hip) ---------------------------------------------------
extern "C" int32_t kmpc_observe_batch(int32_t device, int32_t B, void *rec, const void *z, const void *u, int32_t u_stride, const void *params,
                                      double dt, double L_a, double L_b, double gate, double v_min, double psi_cap, void *est_out, void *dist_out,
                                      void *innov_out, int32_t *flags_out, void *stream)
{
    if (B < 0 || u_stride < 2 || !pos(dt) || !pos(L_a) || !pos(L_b) || !nonneg(gate) || !nonneg(v_min) || !nonneg(psi_cap))
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_observe_batch: bad argument (B=%d, u_stride=%d, dt=%g, L_a=%g, L_b=%g, gate=%g, v_min=%g, psi_cap=%g)", B,
                    u_stride, dt, L_a, L_b, gate, v_min, psi_cap);
    if (B > 0 && (!rec || !z || !u || !params || !est_out)) return fail(nullptr, KMPC_ERR_ARG, "kmpc_observe_batch: null required buffer");
    if (B == 0) return KMPC_OK;
    return on_device("kmpc_observe_batch", device, [&] {
        return kmpc_launch_observe(B, (double *)rec, (const double *)z, (const double *)u, u_stride, (const double *)params, dt, L_a, L_b, gate, v_min, psi_cap,
                                   (double *)est_out, (double *)dist_out, (double *)innov_out, flags_out, (hipStream_t)stream);
    });
}

extern "C" int32_t kmpc_cmd_offset_batch(int32_t device, int32_t B, const void *rec, const uint8_t *stop_latch, double acc_cap, double df_cap,
                                         void *cmd, void *stream)
{
    if (B < 0 || !nonneg(acc_cap) || !nonneg(df_cap))
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_cmd_offset_batch: bad argument (B=%d, acc_cap=%g, df_cap=%g)", B, acc_cap, df_cap);
    if (B > 0 && (!rec || !cmd)) return fail(nullptr, KMPC_ERR_ARG, "kmpc_cmd_offset_batch: null required buffer");
    if (B == 0) return KMPC_OK;
    return on_device("kmpc_cmd_offset_batch", device, [&] {
        return kmpc_launch_cmd_offset(B, (const double *)rec, stop_latch, acc_cap, df_cap, (double *)cmd, (hipStream_t)stream);
    });
}

// ---- prediction ahead under estimated disturbances (kmpc_predict_dist.hip) -------------------------------------------
extern "C" int32_t kmpc_predict_ahead_dist_batch(int32_t device, int32_t B, const void *rec, const void *est, const void *cmd_hist, int32_t depth,
                                                 int64_t period, int32_t n_updates, const int32_t *cmd_delay, const int32_t *meas_delay,
                                                 int32_t max_cmd_delay, int32_t max_meas_delay, double L_a, double L_b, double psi_cap, void *z_out,
                                                 void *stream)
{
    const int32_t rc = latency_args("kmpc_predict_ahead_dist_batch", B, cmd_hist, depth, period, n_updates, cmd_delay, meas_delay, max_cmd_delay,
                                    max_meas_delay);
    if (rc != KMPC_OK) return rc;
    if (!pos(L_a) || !pos(L_b) || !nonneg(psi_cap))
        return fail(nullptr, KMPC_ERR_ARG, "kmpc_predict_ahead_dist_batch: L_a=%g, L_b=%g must be finite and > 0, psi_cap=%g finite and >= 0", L_a, L_b,
                    psi_cap);
    if (B > 0 && (!rec || !est || !z_out)) return fail(nullptr, KMPC_ERR_ARG, "kmpc_predict_ahead_dist_batch: null rec, est or z_out");
    if (B == 0) return KMPC_OK;
    return on_device("kmpc_predict_ahead_dist_batch", device, [&] {
        return kmpc_launch_predict_ahead_dist(B, (const double *)rec, (const double *)est, (const double *)cmd_hist, depth, (long long)period, n_updates, cmd_delay,
                                              meas_delay, max_cmd_delay, max_meas_delay, L_a, L_b, psi_cap, (double *)z_out, (hipStream_t)stream);
    });
}

extern "C" int32_t kmpc_command_batch(int32_t device, int32_t B, const void *u0, const int32_t *stop, uint8_t *stop_latch, void *u_prev, void *cmd, void *stream)
{
    if (B < 0 || (B > 0 && (!u0 || !stop || !stop_latch || !u_prev || !cmd))) return fail(nullptr, KMPC_ERR_ARG, "kmpc_command_batch: bad argument (B=%d)", B);
    if (B == 0) return KMPC_OK;
    return on_device("kmpc_command_batch", device, [&] {
        return kmpc_launch_command(B, (const double *)u0, stop, stop_latch, (double *)u_prev, (double *)cmd, (hipStream_t)stream);
    });
}

// ---- Frenet reference from waypoints (kmpc_frenet_ref.hip) ----------------------------------------------------------
extern "C" int32_t kmpc_frenet_reference_batch(int32_t device, int32_t B, int32_t horizon, const double *pose, const double *ref, const double *v,
                                               double *k_poly, double *psi_start, double *z0, int32_t *fit_status, void *stream)
{
    if (B < 0 || horizon < 2 || horizon > 56) return fail(nullptr, KMPC_ERR_ARG, "kmpc_frenet_reference_batch: bad argument (B=%d, horizon=%d; horizon 2..56)", B, horizon);
    if (B > 0 && (!pose || !ref || !k_poly || !psi_start || !fit_status)) return fail(nullptr, KMPC_ERR_ARG, "kmpc_frenet_reference_batch: null required buffer");
    if (z0 && !v) return fail(nullptr, KMPC_ERR_ARG, "kmpc_frenet_reference_batch: z0 needs v");
    if (B == 0) return KMPC_OK;
    FR f;
    f.B = B; f.H = horizon; f.pose = pose; f.ref = ref; f.v = v; f.k_poly = k_poly; f.psi = psi_start; f.z0 = z0; f.status = fit_status;
    return on_device("kmpc_frenet_reference_batch", device, [&] { return kmpc_launch_frenet_ref(f, (hipStream_t)stream); });
}
