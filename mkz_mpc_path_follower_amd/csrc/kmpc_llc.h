// kmpc_llc.h -- the reference's low-level controller (src/LowLevelController.cpp with PidControl.h and LowPass.h: SURVEY.md section 2, component 11)
// as ONE device function: llc_tick is one recvSteeringReport (:205-226) followed by one controlCallback (:111-198) with sys_enable_ true, for one
// vehicle, fp64, every operation rounded on its own (contraction off), no transcendental: the chain reference classes == numpy restatement ==
// this function holds bit for bit (tests/test_lowlevel_ref.py, tests/test_lowlevel.py).  include/kmpc.h states the arithmetic and the layouts.
// Dropped: PidControl::step's derivative term (kd = 0 in :55: it adds +-0 to y, which changes no comparison and no non-zero y).
// Not modelled: the 0.2 s command timeout (:113-116; the loops publish every period), the fuel low-pass (:46, :118: fuel level 0, the mass is the
// row's), pedals_enable_ / steer_enable_ (:181-188: both on).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/kmpc.h"

#pragma clang fp contract(off)

namespace llc {

// the controller's words of a record row (KMPC_LLCREC_INT ... KMPC_LLCREC_MAX_ERR without the plant's two actuator states), kept in registers
struct state {
    double integ, lpf, ready, v_last;             // PidControl::int_val_, LowPass::last_val_ / ready_ of lpf_accel_, actual_.linear.x
    double th_cmd, br_cmd, wheel_cmd, acc_cmd;    // last published: throttle fraction, brake torque [N m], steering-wheel angle [rad], clamped accel
    double ticks, n_th_sat, n_deadband, n_brake;  // counters
    double sum_err2, max_err;                     // of e = ac - LPF
};

// a parameter row (KMPC_LLC_*)
struct params { double kp, ki, accel_max, decel_max, steer_ratio, mass, brake_deadband, wheel_radius; };

__device__ __forceinline__ state load(const double *__restrict__ r)
{
    return state{r[KMPC_LLCREC_INT], r[KMPC_LLCREC_LPF], r[KMPC_LLCREC_READY], r[KMPC_LLCREC_V_LAST], r[KMPC_LLCREC_TH_CMD], r[KMPC_LLCREC_BR_CMD],
                 r[KMPC_LLCREC_WHEEL_CMD], r[KMPC_LLCREC_ACC_CMD], r[KMPC_LLCREC_TICKS], r[KMPC_LLCREC_N_TH_SAT], r[KMPC_LLCREC_N_DEADBAND],
                 r[KMPC_LLCREC_N_BRAKE], r[KMPC_LLCREC_SUM_ERR2], r[KMPC_LLCREC_MAX_ERR]};
}

__device__ __forceinline__ void store(double *__restrict__ r, const state &s)
{
    r[KMPC_LLCREC_INT] = s.integ; r[KMPC_LLCREC_LPF] = s.lpf; r[KMPC_LLCREC_READY] = s.ready; r[KMPC_LLCREC_V_LAST] = s.v_last;
    r[KMPC_LLCREC_TH_CMD] = s.th_cmd; r[KMPC_LLCREC_BR_CMD] = s.br_cmd; r[KMPC_LLCREC_WHEEL_CMD] = s.wheel_cmd; r[KMPC_LLCREC_ACC_CMD] = s.acc_cmd;
    r[KMPC_LLCREC_TICKS] = s.ticks; r[KMPC_LLCREC_N_TH_SAT] = s.n_th_sat; r[KMPC_LLCREC_N_DEADBAND] = s.n_deadband; r[KMPC_LLCREC_N_BRAKE] = s.n_brake;
    r[KMPC_LLCREC_SUM_ERR2] = s.sum_err2; r[KMPC_LLCREC_MAX_ERR] = s.max_err;
}

__device__ __forceinline__ params load_params(const double *__restrict__ r)
{
    return params{r[KMPC_LLC_KP], r[KMPC_LLC_KI], r[KMPC_LLC_ACCEL_MAX], r[KMPC_LLC_DECEL_MAX], r[KMPC_LLC_STEER_RATIO], r[KMPC_LLC_MASS],
                  r[KMPC_LLC_BRAKE_DEADBAND], r[KMPC_LLC_WHEEL_RADIUS]};
}

// one tick: the speed report `v`, then the control callback on the command (acc_des, df_des)
__device__ __forceinline__ void tick(state &s, const params &p, double v, double acc_des, double df_des)
{
    const double tau = 0.5, ts = 0.02;                       // lpf_accel_.setParams(0.5, 0.02), :47
    const double a = 1 / (tau / ts + 1);                     // LowPass.h:49
    const double b = tau / ts / (tau / ts + 1);              // LowPass.h:50
    const double sample_time = 0.02;                         // control_period_ = 1.0 / 50.0, :60-61
    // recvSteeringReport, :207-219
    const double raw = 50.0 * (v - s.v_last);                // :207
    s.lpf = s.ready != 0.0 ? a * raw + b * s.lpf : raw;      // LowPass::filt, LowPass.h:53-61
    s.ready = 1.0;
    s.v_last = v;                                            // :219
    // controlCallback, :120-179
    const double ac = acc_des > p.accel_max ? p.accel_max : (acc_des < -p.decel_max ? -p.decel_max : acc_des);   // :123-128
    const double e = ac - s.lpf;                             // :145, :148
    double th = 0.0;
    if (ac >= 0) {                                           // :147: PidControl::step(e, control_period_), PidControl.h:63-79
        const double integral = s.integ + e * sample_time;   // PidControl.h:66
        double y = p.kp * e + p.ki * s.integ;                // PidControl.h:69: the OLD integrator
        if (y > 1.0) {                                       // setRange(0.0, 1.0), :56
            y = 1.0;
            s.n_th_sat = s.n_th_sat + 1.0;
        } else if (y < 0.0) {
            y = 0.0;
        } else {
            s.integ = integral;                              // PidControl.h:75: conditional integration
        }
        th = y;
    } else {
        s.integ = 0.0;                                       // :150 resetIntegrator
        if (ac >= -p.brake_deadband) s.n_deadband = s.n_deadband + 1.0;
    }
    double br = 0.0;
    if (ac < -p.brake_deadband) {                            // :156
        br = -ac * p.mass * p.wheel_radius;                  // :157 [N m]
        s.n_brake = s.n_brake + 1.0;
    }
    double w = df_des * p.steer_ratio;                       // :164
    if (fabs(w) > 8.2) w = w > 0.0 ? 8.2 : -8.2;             // :175-177, STEER_MAX
    s.th_cmd = th; s.br_cmd = br; s.wheel_cmd = w; s.acc_cmd = ac;
    s.ticks = s.ticks + 1.0;
    s.sum_err2 = s.sum_err2 + e * e;
    s.max_err = fabs(e) > s.max_err ? fabs(e) : s.max_err;
}

}   // namespace llc
