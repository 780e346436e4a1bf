"""mkz_mpc_path_follower_amd -- MI355X-native batched kinematic-bicycle MPC solver.

Drop-in for ONE path of govvijaycal/mkz_mpc_path_follower: the per-step nonlinear MPC solve of
scripts/mpc_utils/MKZMPCPathFollower.jl as driven by scripts/mpc_cmd_pub.jl.  Importing the
package does not touch the GPU; constructing a solver does, and fails loudly without one.
"""
__all__ = ["BatchMPC", "KinematicMPC", "synthetic", "get_reference_frenet_batch", "ClosedLoopFrenet", "ClosedLoop", "FleetRefTrajectory", "SpeedPlanner"]


def __getattr__(name):
    if name == "BatchMPC":
        from .solver import BatchMPC
        return BatchMPC
    if name == "KinematicMPC":
        from .kinematic_mpc import KinematicMPC
        return KinematicMPC
    if name == "get_reference_frenet_batch":
        from .kinematic_mpc_frenet import get_reference_frenet_batch
        return get_reference_frenet_batch
    if name == "ClosedLoopFrenet":
        from .closed_loop import ClosedLoopFrenet
        return ClosedLoopFrenet
    if name == "ClosedLoop":
        from .closed_loop import ClosedLoop
        return ClosedLoop
    if name == "FleetRefTrajectory":
        from .ref_traj import FleetRefTrajectory
        return FleetRefTrajectory
    if name == "SpeedPlanner":
        from .ref_traj import SpeedPlanner
        return SpeedPlanner
    if name == "synthetic":
        from . import synthetic
        return synthetic
    raise AttributeError(name)
