"""The Frenet node's loop on the CPU (test helper; uses oracle/ -- test infrastructure).

scripts/nodes_gazebo_sim/gazebo_sim_mpc_cmd_pub_frenet.jl:54-153 for ONE vehicle with the waypoint helper in the place of the path topic: the oracle's
get_waypoints at a target speed -> the path in the vehicle frame with the origin in front (convert_msg_to_path_dict, :54-85) -> the numpy curvature fit
(nav_msgs_path_frenet.py:62-86, the package's single-vehicle get_reference_frenet) -> update_init_cond(0, 0, -psi_start, v) (:128) -> the oracle's Frenet
solve, warm from the second step on -> the oracle's plant.  The GPU loop (closed_loop.ClosedLoopFrenet) is compared against it.
"""
import math
import warnings

import numpy as np

from scenario import cross_track, path_arrays  # noqa: F401  (re-exported for the tests)

FRENET_WEIGHTS = (0.0, 9.0, 10.0, 0.5, 100.0, 1000.0, 0.0, 0.0)   # MKZMPCPathFollowerFrenet.jl:51-59 in the 8-slot layout


def vehicle_frame_path(pose, xr, yr):
    """convert_msg_to_path_dict (:54-85): global waypoints -> dict(x, y, s) in the frame of pose = (x, y, yaw), (0, 0) at s = 0 in front, s the
    SEQUENTIAL cumulative chord length (first increment: origin -> first waypoint)"""
    X0, Y0, yaw = (float(a) for a in pose)
    c, s_ = math.cos(yaw), math.sin(yaw)
    dx, dy = np.asarray(xr, dtype=np.float64) - X0, np.asarray(yr, dtype=np.float64) - Y0
    x = np.concatenate([[0.0], c * dx + s_ * dy])
    y = np.concatenate([[0.0], c * dy - s_ * dx])
    s = np.zeros(len(x))
    acc = 0.0
    for i in range(1, len(x)):
        acc = acc + math.sqrt((x[i] - x[i - 1]) ** 2 + (y[i] - y[i - 1]) ** 2)
        s[i] = acc
    return dict(x=x, y=y, s=s)


def numpy_reference(path):
    """get_reference_frenet (nav_msgs_path_frenet.py:76-86) -> (K_coeffs highest degree first, psi_start); a RankWarning is an error here"""
    from mkz_mpc_path_follower_amd.kinematic_mpc_frenet import get_reference_frenet
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        K, psi, _, _ = get_reference_frenet(path)
    return np.asarray(K, dtype=np.float64), float(psi)


def grid_margin(s_end):
    """distance of s_end / 0.5 and s_end / 0.25 from the nearest integer: the lengths of the two np.arange grids hinge on them"""
    return min(abs(s_end / 0.5 - round(s_end / 0.5)), abs(s_end / 0.25 - round(s_end / 0.25)))


def oracle_frenet_loop(O, steps, path="path1_decimated.npz", target_vel=5.0, X0=0.0, Y0=0.0, Psi0=0.0, v0=0.0, N=8):
    """-> dict of per-step arrays: state [steps+1, 8], cmd [steps, 2], status, iters, stop (latched), k_poly [steps, 4], psi_start; traj"""
    from oracle import waypoints as W, vehicle_sim as V
    arr, lat0, lon0 = path_arrays(path)
    traj = W.build_trajectory(arr["t"], arr["lat"], arr["lon"], arr["psi"], lat0, lon0)
    p = O.params(N, FRENET_WEIGHTS, model=1)
    s = V.initial_state(1, X0, Y0, Psi0)
    s[0, 3] = v0
    u_prev = np.zeros(2)
    U_prev, have_warm, command_stop = None, False, False
    log = dict(state=[s[0].copy()], cmd=[], status=[], iters=[], stop=[], k_poly=[], psi_start=[])
    for _ in range(steps):
        x, y, psi, v = s[0, 0], s[0, 1], s[0, 2], s[0, 3]
        xr, yr, _pr, stop, _ci = W.get_waypoints(traj, x, y, psi, target_vel, traj_horizon=N)
        command_stop = command_stop or stop
        if not command_stop:
            K, psi_start = numpy_reference(vehicle_frame_path((x, y, psi), xr, yr))
            q = O.problem_frenet(p, [0.0, 0.0, -psi_start, v], K, target_vel, u_prev)   # :128-129
            r = O.solve_condensed(p, q, o=O.opts(warm=1) if have_warm else O.opts(), U0=U_prev)
            cmd = r["U"][0].copy()
            u_prev = cmd.copy()                                                         # :149
            U_prev, have_warm = r["U"].copy(), True
            log["status"].append(r["status"]); log["iters"].append(r["iters"]); log["k_poly"].append(K); log["psi_start"].append(psi_start)
        else:
            cmd = np.array([-1.0, 0.0])
            log["status"].append(-1); log["iters"].append(0); log["k_poly"].append(np.zeros(4)); log["psi_start"].append(0.0)
        log["cmd"].append(cmd); log["stop"].append(command_stop)
        s = V.update_vehicle_model(s, cmd[None, :], n_updates=10)
        log["state"].append(s[0].copy())
    out = {k: np.array(v) for k, v in log.items()}
    out["traj"] = traj
    return out
