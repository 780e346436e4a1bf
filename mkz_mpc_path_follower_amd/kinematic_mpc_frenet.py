"""Single-problem mirror of the reference's Julia module scripts/mpc_utils/MKZMPCPathFollowerFrenet.jl and of the
curvature-polynomial fit that feeds it (scripts/sim_path_utils/nav_msgs_path_frenet.py:44-86).

Same six functions, same argument orders: update_init_cond(s, ey, epsi, vel) (:132-138), update_reference(path, k_coeffs,
v_des) (:142-147), update_current_input(c_swa, c_acc) -- steer first (:151-154), update_cost(cey, cep, cev, cda, cdd, ca, cd)
(:158-169), solve_model() -> (acc, d_f, status) (:173-183), get_solver_results() -> (s, ey, v, epsi, K, path_ref, d_f, acc)
(:188-207, v before epsi, d_f before acc).  The solve runs on the MI355X (kmpc_solve_batch_frenet, B = 1); no CPU path.

get_reference_frenet_batch is the fleet form of the fit: vehicle-frame path, curvature polynomial and initial condition for B vehicles in one
kernel on the device (kmpc_frenet_reference_batch), from the waypoints kmpc_waypoints_batch wrote.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import STATUS_NAMES
from .solver import BatchMPC


# ---- curvature-polynomial fit of nav_msgs_path_frenet.py:44-86 (numpy's polynomial helpers, coefficients highest degree first) --------
def fit_XY_s(x_arr, y_arr, s_arr):
    """:62-73  X(s), Y(s) cubics through the waypoints resampled every 0.5 m"""
    s_interp = np.arange(s_arr[0], s_arr[-1], 0.5)
    x_interp = np.interp(s_interp, s_arr, x_arr)
    y_interp = np.interp(s_interp, s_arr, y_arr)
    return np.polyfit(s_interp, x_interp, 3), np.polyfit(s_interp, y_interp, 3)


def compute_curvature_poly(s_interp, x_coeffs, y_coeffs):
    """:44-59  K = (x' y'' - y' x'') / (x'^2 + y'^2) on the fitted cubics, then a cubic fit of K(s), highest degree first"""
    s_interp = np.asarray(s_interp, dtype=np.float64)
    d1x, d1y = np.polyder(x_coeffs), np.polyder(y_coeffs)
    dx, dy = np.polyval(d1x, s_interp), np.polyval(d1y, s_interp)
    ddx, ddy = np.polyval(np.polyder(d1x), s_interp), np.polyval(np.polyder(d1y), s_interp)
    K_meas = (dx * ddy - dy * ddx) / (dx ** 2 + dy ** 2)
    return np.polyfit(s_interp, K_meas, 3)


def get_reference_frenet(path):
    """:76-86  path = dict(x, y, s) -> (K_coeffs, psi_start, x_interp, y_interp)"""
    x_coeffs, y_coeffs = fit_XY_s(path["x"], path["y"], path["s"])
    s_interp = np.arange(0.0, path["s"][-1], 0.25)
    x_interp = np.polyval(x_coeffs, s_interp)
    y_interp = np.polyval(y_coeffs, s_interp)
    K_coeffs = compute_curvature_poly(s_interp, x_coeffs, y_coeffs)
    psi_start = math.atan2(y_coeffs[2], x_coeffs[2])   # slopes of the two cubics at s = 0
    return K_coeffs, psi_start, x_interp, y_interp


def get_reference_frenet_batch(pose, ref, v=None):
    """gazebo_sim_mpc_cmd_pub_frenet.jl:54-85 (path in the vehicle frame, origin in front, cumulative chord length) + get_reference_frenet
    (:76-86) + the arguments of update_init_cond (:128) for B vehicles on the device.
    pose [B,3] (x, y, yaw), ref [B,H+1,3] (GPSRefTrajectory.get_waypoints_batch's output, H = 2..56), v [B] measured speeds or None
    -> k_poly [B,4] (highest degree first), psi_start [B], z0 [B,4] = (0, 0, -psi_start, v) (None without v), fit_status [B] int32
    (0 fitted; 1 refused: fewer than four 0.5 m resample points, a non-finite value, or a window longer than 8192 m -- zeros then).
    float64 device tensors; asynchronous on torch's current stream.  No CPU fallback."""
    if not torch.cuda.is_available():
        raise RuntimeError("get_reference_frenet_batch needs an MI355X; no CPU fallback")
    ref = torch.as_tensor(ref, dtype=torch.float64)
    dev = ref.device if ref.is_cuda else (pose.device if isinstance(pose, torch.Tensor) and pose.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    ref = ref.to(dev).contiguous()
    pose = torch.as_tensor(pose, dtype=torch.float64, device=dev).contiguous()
    if pose.dim() != 2 or pose.shape[1] != 3:
        raise ValueError("pose: expected [B,3], got %s" % (tuple(pose.shape),))
    B = pose.shape[0]
    if ref.dim() != 3 or ref.shape[0] != B or ref.shape[2] != 3 or not 2 <= ref.shape[1] - 1 <= 56:
        raise ValueError("ref: expected [%d,H+1,3] with H = 2..56, got %s" % (B, tuple(ref.shape)))
    if v is not None:
        v = torch.as_tensor(v, dtype=torch.float64, device=dev).contiguous()
        if tuple(v.shape) != (B,):
            raise ValueError("v: expected [%d], got %s" % (B, tuple(v.shape)))
    k_poly = torch.empty((B, 4), dtype=torch.float64, device=dev)
    psi_start = torch.empty((B,), dtype=torch.float64, device=dev)
    z0 = torch.empty((B, 4), dtype=torch.float64, device=dev) if v is not None else None
    fit_status = torch.empty((B,), dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.load().kmpc_frenet_reference_batch(dev.index, B, ref.shape[1] - 1, p(pose), p(ref), p(v), p(k_poly), p(psi_start), p(z0),
                                                       p(fit_status), stream))
    return k_poly, psi_start, z0, fit_status


class KinematicMPCFrenet:
    dt_control = 0.10  # MKZMPCPathFollowerFrenet.jl:28
    dt = 0.20          # :33

    def __init__(self, N=8, device=0, **options):
        self.N = int(N)  # :34
        self._mpc = BatchMPC(N=self.N, dtype=torch.float64, device=device, model=1, **options)
        self._z0 = np.zeros((1, 4))                 # s0, ey0, epsi0, v0 (:107-110)
        self._kp = np.zeros((1, 4))                 # k_coeff_ref (:38)
        self._vt = np.array([15.0])                 # v_ref (:37)
        self._up = np.zeros((1, 2))                 # (acc_current, d_f_current)
        self._U = np.zeros((self.N, 2))
        self._X = np.zeros((self.N + 1, 4))
        self._warm = None
        self.path_ref = {}                          # :36
        self.status = self.cost = self.iters = None
        self.solve_model()                          # the module solves once at load time (:125-128)

    def close(self):
        self._mpc.close()

    def update_init_cond(self, s, ey, epsi, vel):   # :132-138
        self._z0[0, :] = (s, ey, epsi, vel)

    def update_reference(self, path, k_coeffs, v_des):  # :142-147
        k = np.asarray(k_coeffs, dtype=np.float64).ravel()
        if k.shape != (4,):
            raise ValueError("k_coeffs must have 4 entries, highest degree first")
        self.path_ref = path
        self._kp[0, :] = k
        self._vt[0] = float(v_des)

    def update_current_input(self, c_swa, c_acc):   # :151-154 (steer first)
        self._up[0, :] = (c_acc, c_swa)

    def update_cost(self, cey, cep, cev, cda, cdd, ca, cd):  # :158-169
        self._mpc.update_cost(0.0, cey, cep, cev, cda, cdd, ca, cd)

    def solve_model(self):                          # :173-183
        warm = self._warm is not None
        wu = self._warm if warm else torch.zeros((1, self.N, 2), dtype=torch.float64, device=self._mpc.device)
        o = self._mpc.solve_frenet(self._z0, self._kp, self._vt, self._up, warm_U=wu, warm=warm, want_U=True, want_X=True)
        torch.cuda.synchronize(self._mpc.device)
        self._warm = o["warm_U"]                    # JuMP re-solves from the previous primal values (Q9)
        self._U = o["U"][0].cpu().numpy()
        self._X = o["X"][0].cpu().numpy()
        self.status = STATUS_NAMES[int(o["status"][0].item())]
        self.cost, self.iters = float(o["cost"][0].item()), int(o["iters"][0].item())
        return float(self._U[0, 0]), float(self._U[0, 1]), self.status

    def get_solver_results(self):                   # :188-207
        X, U = self._X, self._U
        return (X[:, 0].copy(), X[:, 1].copy(), X[:, 3].copy(), X[:, 2].copy(), self._kp[0].copy(), self.path_ref,
                U[:, 1].copy(), U[:, 0].copy())
