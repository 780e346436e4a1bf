"""ctypes binding of the C ABI in include/kmpc.h (libkmpc_hip.so, built for gfx950).

There is no CPU fallback: if the shared library is missing or cannot be loaded this module
raises, and every compute entry point fails when no MI355X is present.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libkmpc_hip.so")

KMPC_F64, KMPC_F32 = 0, 1
STATUS_NAMES = {0: "Optimal", 1: "UserLimit", 2: "Infeasible", 3: "Error"}  # cf. JuMP status symbols


class Config(C.Structure):
    """struct kmpc_config (include/kmpc.h) = constants of MKZMPCPathFollower.jl:28-48 + solver options."""
    _fields_ = [("N", C.c_int32), ("dtype", C.c_int32),
                ("dt", C.c_double), ("dt_control", C.c_double), ("L_a", C.c_double), ("L_b", C.c_double),
                ("steer_max", C.c_double), ("steer_dmax", C.c_double), ("a_max", C.c_double),
                ("a_dmax", C.c_double), ("v_min", C.c_double), ("v_max", C.c_double),
                ("max_iter", C.c_int32), ("hessian", C.c_int32), ("tol", C.c_double),
                ("mu_init", C.c_double), ("bound_relax", C.c_double), ("warm_push", C.c_double),
                ("warm_mu", C.c_double), ("max_ls", C.c_int32), ("kernel_variant", C.c_int32),
                ("mu_strategy", C.c_int32), ("indef_strategy", C.c_int32), ("schedule", C.c_int32), ("model", C.c_int32),
                ("start", C.c_int32)]


EXPORTS = ["kmpc_abi_version", "kmpc_config_default", "kmpc_create", "kmpc_destroy", "kmpc_set_cost",
           "kmpc_get_cost", "kmpc_solve_batch", "kmpc_solve_batch_host", "kmpc_last_error",
           "kmpc_debug_condense", "kmpc_debug_mfma_probe",
           "kmpc_path_create", "kmpc_path_destroy", "kmpc_waypoints_batch", "kmpc_path_last_error",
           "kmpc_sim_advance_batch", "kmpc_solve_batch_frenet", "kmpc_debug_kkt", "kmpc_command_batch",
           "kmpc_record_bytes", "kmpc_pack_records", "kmpc_solve_batch_packed",
           "kmpc_get_problem_params", "kmpc_solve_batch_params", "kmpc_solve_batch_frenet_params",
           "kmpc_frenet_reference_batch",
           "kmpc_pathset_create", "kmpc_pathset_destroy", "kmpc_waypoints_fleet", "kmpc_pathset_last_error",
           "kmpc_track_score_init", "kmpc_track_score_batch", "kmpc_track_score_fleet",
           "kmpc_plant_default", "kmpc_sim_advance_plant", "kmpc_sense_batch", "kmpc_estimate_batch",
           "kmpc_sim_advance_queue", "kmpc_sense_delayed_batch", "kmpc_cmd_in_force_batch", "kmpc_predict_ahead_batch",
           "kmpc_road_default", "kmpc_sim_advance_road", "kmpc_observe_batch", "kmpc_cmd_offset_batch",
           "kmpc_predict_ahead_dist_batch",
           "kmpc_llc_default", "kmpc_llc_step_batch", "kmpc_drive_default", "kmpc_sim_advance_drive",
           "kmpc_pathset_curvature", "kmpc_speed_plan_default", "kmpc_speed_plan_fleet",
           "kmpc_road_profile_default", "kmpc_road_profile_fleet", "kmpc_speed_plan_fleet_profile",
           "kmpc_sense_faults_default", "kmpc_sense_faults_batch",
           "kmpc_wander_default", "kmpc_wander_batch"]
# the entry points of include/kmpc_follow.h: the same library, a header of their own (EXPORTS is include/kmpc.h's list and stays that)
EXT_EXPORTS = ["kmpc_follow_default", "kmpc_follow_stat_init", "kmpc_follow_fleet"]
# the entry points of include/kmpc_lanes.h, likewise a list of their own
LANE_EXPORTS = ["kmpc_lane_default", "kmpc_lane_rec_init", "kmpc_lane_step_fleet", "kmpc_ref_offset_batch"]
# the entry points of include/kmpc_range.h, likewise
RANGE_EXPORTS = ["kmpc_range_default", "kmpc_range_rec_init", "kmpc_range_follow_batch"]
# the entry points of include/kmpc_order.h, likewise
ORDER_EXPORTS = ["kmpc_order_bytes", "kmpc_order_fleet", "kmpc_order_follow_fleet", "kmpc_order_lane_step_fleet"]

_lib = None


def load():
    """Load libkmpc_hip.so; raise (never fall back) if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int32
    L.kmpc_abi_version.restype = i32
    L.kmpc_config_default.argtypes = [C.POINTER(Config), i32, i32]
    L.kmpc_create.argtypes = [C.POINTER(Config), i32, C.POINTER(vp)]
    L.kmpc_destroy.argtypes = [vp]
    L.kmpc_set_cost.argtypes = [vp, C.POINTER(C.c_double)]
    L.kmpc_get_cost.argtypes = [vp, C.POINTER(C.c_double)]
    sig = [vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.kmpc_solve_batch.argtypes = sig + [vp]
    L.kmpc_solve_batch_host.argtypes = sig
    L.kmpc_solve_batch_frenet.argtypes = sig + [vp]
    sig_par = sig[:6] + [vp] + sig[6:] + [vp]   # params [B,16] behind u_prev
    L.kmpc_solve_batch_params.argtypes = sig_par
    L.kmpc_solve_batch_frenet_params.argtypes = sig_par
    L.kmpc_get_problem_params.argtypes = [vp, C.POINTER(C.c_double)]
    L.kmpc_last_error.argtypes = [vp]
    L.kmpc_last_error.restype = C.c_char_p
    L.kmpc_debug_condense.argtypes = [vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    L.kmpc_debug_mfma_probe.argtypes = [vp, vp, vp, vp, vp]
    L.kmpc_debug_kkt.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, C.c_double, C.c_double, i32, vp, vp, vp, vp, vp]
    dp = C.POINTER(C.c_double)
    L.kmpc_path_create.argtypes = [i32, i32, dp, dp, dp, dp, dp, C.POINTER(vp)]
    L.kmpc_path_destroy.argtypes = [vp]
    L.kmpc_waypoints_batch.argtypes = [vp, i32, i32, C.c_double, vp, vp, vp, vp, vp, vp]
    L.kmpc_path_last_error.argtypes = [vp]
    L.kmpc_path_last_error.restype = C.c_char_p
    L.kmpc_pathset_create.argtypes = [i32, i32, C.POINTER(i32), dp, dp, dp, dp, dp, C.POINTER(vp)]
    L.kmpc_pathset_destroy.argtypes = [vp]
    L.kmpc_waypoints_fleet.argtypes = [vp, i32, i32, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp]
    L.kmpc_pathset_last_error.argtypes = [vp]
    L.kmpc_pathset_last_error.restype = C.c_char_p
    L.kmpc_track_score_init.argtypes = [dp, i32]
    L.kmpc_track_score_batch.argtypes = [vp, i32, vp, i32, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.kmpc_track_score_fleet.argtypes = [vp, i32, vp, i32, vp, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.kmpc_pathset_curvature.argtypes = [vp, C.c_double, vp, vp]
    L.kmpc_speed_plan_default.argtypes = [dp, i32]
    L.kmpc_speed_plan_fleet.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.kmpc_road_profile_default.argtypes = [dp, i32]
    L.kmpc_road_profile_fleet.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp, vp, vp]
    L.kmpc_speed_plan_fleet_profile.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.kmpc_sim_advance_batch.argtypes = [i32, i32, vp, vp, i32, vp]
    L.kmpc_plant_default.argtypes = [dp]
    L.kmpc_sim_advance_plant.argtypes = [i32, i32, vp, vp, vp, vp, vp, i32, vp]
    L.kmpc_sense_batch.argtypes = [i32, i32, vp, vp, C.c_uint64, C.c_int64, C.c_int64, vp, vp]
    L.kmpc_estimate_batch.argtypes = [i32, i32, vp, vp, vp, i32, vp, C.c_double, C.c_double, C.c_double, C.c_double, vp, vp, vp, vp]
    L.kmpc_observe_batch.argtypes = [i32, i32, vp, vp, vp, i32, vp] + [C.c_double] * 6 + [vp, vp, vp, vp, vp]
    L.kmpc_cmd_offset_batch.argtypes = [i32, i32, vp, vp, C.c_double, C.c_double, vp, vp]
    L.kmpc_sim_advance_queue.argtypes = [i32, i32, vp, vp, vp, vp, vp, i32, C.c_int64, i32, vp]
    L.kmpc_road_default.argtypes = [dp]
    L.kmpc_sim_advance_road.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp, i32, C.c_int64, i32, vp, vp]
    L.kmpc_llc_default.argtypes = [dp]
    L.kmpc_drive_default.argtypes = [dp]
    L.kmpc_llc_step_batch.argtypes = [i32, i32, vp, vp, i32, vp, vp, vp, vp]
    L.kmpc_sim_advance_drive.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, C.c_int64, i32, vp, vp]
    L.kmpc_sense_delayed_batch.argtypes = [i32, i32, vp, vp, C.c_uint64, C.c_int64, C.c_int64, vp, vp, i32, vp, vp]
    L.kmpc_sense_faults_default.argtypes = [dp, i32]
    L.kmpc_sense_faults_batch.argtypes = [i32, i32, vp, vp, vp, C.c_uint64, C.c_int64, C.c_int64, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.kmpc_wander_default.argtypes = [dp, i32]
    L.kmpc_wander_batch.argtypes = [i32, i32, vp, vp, C.c_uint64, C.c_int64, C.c_int64, vp, vp, vp, vp, vp]
    L.kmpc_cmd_in_force_batch.argtypes = [i32, i32, vp, i32, C.c_int64, i32, vp, vp, i32, i32, vp, vp]
    L.kmpc_predict_ahead_batch.argtypes = [i32, i32, vp, vp, i32, C.c_int64, i32, vp, vp, i32, i32, C.c_double, C.c_double, vp, vp]
    L.kmpc_predict_ahead_dist_batch.argtypes = [i32, i32, vp, vp, vp, i32, C.c_int64, i32, vp, vp, i32, i32] + [C.c_double] * 3 + [vp, vp]
    L.kmpc_command_batch.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp]
    L.kmpc_frenet_reference_batch.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.kmpc_record_bytes.argtypes = [i32, i32]
    L.kmpc_record_bytes.restype = C.c_int64
    L.kmpc_pack_records.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    L.kmpc_solve_batch_packed.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp, vp]
    L.kmpc_follow_default.argtypes = [dp, i32]
    L.kmpc_follow_stat_init.argtypes = [dp, i32]
    L.kmpc_follow_fleet.argtypes = [i32, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.kmpc_lane_default.argtypes = [dp, i32]
    L.kmpc_lane_rec_init.argtypes = [dp, i32]
    L.kmpc_lane_step_fleet.argtypes = [i32, i32, i32, C.c_double, vp, i32, vp, i32, vp, i32] + [vp] * 13
    L.kmpc_ref_offset_batch.argtypes = [i32, i32, i32, vp, vp, i32, vp]
    L.kmpc_range_default.argtypes = [dp, i32]
    L.kmpc_range_rec_init.argtypes = [dp, i32]
    L.kmpc_range_follow_batch.argtypes = [i32, i32, C.c_double, vp, vp, vp, i32, vp, i32, vp, vp, C.c_uint64, C.c_int64, C.c_int64, vp, vp, vp, vp, vp]
    L.kmpc_order_bytes.argtypes = [i32, i32, C.POINTER(C.c_int64)]
    L.kmpc_order_fleet.argtypes = [i32, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp, C.c_int64, vp]
    L.kmpc_order_follow_fleet.argtypes = L.kmpc_follow_fleet.argtypes[:-1] + [vp, vp]                              # ..., order, stream
    L.kmpc_order_lane_step_fleet.argtypes = L.kmpc_lane_step_fleet.argtypes[:-1] + [vp, i32, vp, C.c_int64, vp]    # ..., order, lanes_max, workspace, bytes, stream
    for name in EXPORTS + EXT_EXPORTS + LANE_EXPORTS + RANGE_EXPORTS + ORDER_EXPORTS:
        getattr(L, name)
    _lib = L
    return L


class KmpcError(RuntimeError):
    pass


def check(rc, handle=None):
    if rc != 0:
        msg = load().kmpc_last_error(handle)
        raise KmpcError("kmpc error %d: %s" % (rc, msg.decode() if msg else "?"))
