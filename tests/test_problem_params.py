"""Per-problem cost weights and limits in one batched solve (kmpc_solve_batch_params / BatchMPC.solve(..., params=); include/kmpc.h).

update_cost (MKZMPCPathFollower.jl:158-169) and the limits steer_max ... v_max (:41-48) are per handle in the reference and in the plain entry points; the
`params` record [B,16] sets them per problem.  The parameter sets come from synthetic.make_param_sets (G seeded sets; problem i of a batch carries set i % G and
its v0 is lowered to min(v0, v_max_i - 0.5)), on make_batch(B, N, cfg_id=2, seed=5100 + N) for the Cartesian model and tests/test_frenet.py::_cases(B, N,
seed=700 + N) for the Frenet functor, sets from seed + 1.  Checked on the CPU with the condensed port under per-set oracle.params: every problem of these draws is
Optimal (test 1 keeps that under test for N = 8 and 20).

CPU:  1  generator, record layout, the port is all-Optimal on the draws the GPU tests rely on.
GPU:  2  same kernel, same answer: a batch of 8 interleaved sets through `params` against per-set handles (kmpc_set_cost + kmpc_config limits) on the SAME full
         batch (so both calls run the same kernel; only the set's rows are compared): u0, U, X, cost, viol, status, iters bit-identical, every back-end.
      3  params = the handle's values is the plain call, bit for bit; params=None goes through the old symbol.
      4  independent certification of every solution under ITS OWN parameters at the bounds tests/test_certify.py uses for the horizon (STRICT 1e-6, 2e-6 from
         N = 28; REFERENCE 1e-7); violation <= bound_relax * max(1, v_max_i) + 1e-12 (the relaxation is relative to the bound: ipm::form_bounds).
      5  invalid records (NaN / negative weight, v_max <= v_min, non-zero reserved slot): status 3, iters 0, zero outputs, nobody else disturbed; a valid record
         that makes the problem infeasible reports what the handle-level limit reports.
      6  limits bite: no problem exceeds its own relaxed v_max; set 3 of the N = 20 draw (v_max = 9.81) has the speed row active on >= 20 problems which exceed it
         when solved under the default v_max.
      7  a mixed fleet in ClosedLoop equals, vehicle by vehicle, the homogeneous loops whose handles carry the sets.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import certify as CT  # noqa: E402
from test_frenet import _cases  # noqa: E402
from mkz_mpc_path_follower_amd.synthetic import LIMIT_NAMES, PARAM_BASE, apply_param_sets, make_batch, make_param_sets, param_records  # noqa: E402

G = 8
KEYS = ("u0", "U", "X", "cost", "viol", "status", "iters")


def _draw(N, B, model=0, dtype=np.float64):
    """(inputs dict with z0, second (ref or k_poly), v_target, u_prev; sets; records [B,16])"""
    if model == 0:
        seed = 5100 + N
        d = make_batch(B, N, cfg_id=2, seed=seed)
        d = dict(z0=d["z0"], second=d["ref"], v_target=d["v_target"], u_prev=d["u_prev"])
    else:
        seed = 700 + N
        z0, kp, vt, up = _cases(B, N, seed=seed)
        d = dict(z0=z0, second=kp, v_target=vt, u_prev=up)
    sets = make_param_sets(G, seed + 1, model=model)
    rec = apply_param_sets(d, sets)
    d = {k: np.ascontiguousarray(v, dtype=dtype) for k, v in d.items()}
    return d, sets, rec.astype(dtype)


# ------------------------------------------------------------------------------------------------------------------------------------ CPU
def test_param_sets_are_deterministic_and_in_range():
    for model in (0, 1):
        a, b = make_param_sets(G, 5121, model=model), make_param_sets(G, 5121, model=model)
        assert len(a) == G
        for (wa, la), (wb, lb) in zip(a, b):
            assert np.array_equal(wa, wb) and la == lb
            nz = wa > 0
            assert (wa[nz] >= PARAM_BASE[nz] * 0.1 - 1e-15).all() and (wa[nz] <= PARAM_BASE[nz] * 10.0 + 1e-12).all()
            assert nz[[1, 2, 4, 5]].all() and (nz[0] or model == 1)                      # pose and rate weights are never zero
            assert 0.35 <= la["steer_max"] <= 0.5 and 0.3 <= la["steer_dmax"] <= 0.5 and 0.8 <= la["a_max"] <= 1.0
            assert 1.2 <= la["a_dmax"] <= 1.5 and la["v_min"] == 0.0 and 9.0 <= la["v_max"] <= 20.0
            assert 0.6 * la["a_max"] < la["a_dmax"] and 0.5 < la["a_max"] and 0.10 < la["a_dmax"] * 0.1   # make_batch's feasibility argument, the start point's proof
    assert not np.array_equal(make_param_sets(G, 5121)[0][0], make_param_sets(G, 5122)[0][0])
    # N = 20 draw: exactly one set has its speed limit below some of its targets (test 6)
    d, sets, rec = _draw(20, 1024)
    below = [int((d["v_target"][g::G] > sets[g][1]["v_max"]).sum()) for g in range(G)]
    assert [g for g in range(G) if below[g]] == [3] and below[3] == 26 and abs(sets[3][1]["v_max"] - 9.81) < 5e-3, (below, sets[3][1])
    assert (d["z0"][:, 3] <= rec[:, 13] - 0.5 + 1e-15).all()


def test_record_layout():
    from mkz_mpc_path_follower_amd.solver import BatchMPC as M
    assert M.P_RECORD == 16 and M.P_WEIGHTS == slice(0, 8) and M.P_RESERVED == slice(14, 16)
    assert (M.P_STEER_MAX, M.P_STEER_DMAX, M.P_A_MAX, M.P_A_DMAX, M.P_V_MIN, M.P_V_MAX) == (8, 9, 10, 11, 12, 13)
    assert LIMIT_NAMES == ("steer_max", "steer_dmax", "a_max", "a_dmax", "v_min", "v_max")
    sets = make_param_sets(3, 1)
    rec = param_records(sets, 7)
    assert rec.shape == (7, 16) and (rec[:, 14:] == 0).all()
    for i in range(7):
        w, lim = sets[i % 3]
        assert np.array_equal(rec[i, M.P_WEIGHTS], w) and rec[i, M.P_V_MAX] == lim["v_max"] and rec[i, M.P_STEER_MAX] == lim["steer_max"]
        assert rec[i, M.P_STEER_DMAX] == lim["steer_dmax"] and rec[i, M.P_A_MAX] == lim["a_max"] and rec[i, M.P_A_DMAX] == lim["a_dmax"] and rec[i, M.P_V_MIN] == 0.0
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kmpc.h")).read()
    for sym in ("kmpc_get_problem_params", "kmpc_solve_batch_params", "kmpc_solve_batch_frenet_params"):
        assert sym in hdr
    assert "[8] steer_max  [9] steer_dmax  [10] a_max  [11] a_dmax  [12] v_min  [13] v_max" in hdr and "0.6 a_max < a_dmax" in hdr


@pytest.mark.parametrize("N,B", [(8, 1024), (20, 1024)])
def test_port_is_all_optimal_on_the_draws(oracle, N, B):
    """the condition tests 2, 4 and 6 rely on: under per-set parameters every problem of the draw has an Optimal solution on the CPU port"""
    O = oracle
    d, sets, rec = _draw(N, B)
    for g, (w, lim) in enumerate(sets):
        p = O.params(N, list(w), **lim)
        r = O.solve_condensed_batch(p, d["z0"][g::G], d["second"][g::G], d["v_target"][g::G], d["u_prev"][g::G], nthreads=8)
        assert (r["status"] == 0).all(), (N, g, np.bincount(r["status"]), r["iters"].max())


@pytest.mark.parametrize("N,B", [(8, 512), (20, 256)])
def test_port_is_all_optimal_on_the_frenet_draws(oracle, N, B):
    O = oracle
    d, sets, rec = _draw(N, B, model=1)
    for g, (w, lim) in enumerate(sets):
        p = O.params(N, list(w), model=1, **lim)
        for i in range(g, B, G):
            r = O.solve_condensed(p, O.problem_frenet(p, d["z0"][i], d["second"][i], d["v_target"][i], d["u_prev"][i]))
            assert r["status"] == 0, (N, g, i, r["status"])


# ------------------------------------------------------------------------------------------------------------------------------------ GPU
def _mpc(N, f32=False, model=0, weights=None, **kw):
    import torch
    from mkz_mpc_path_follower_amd import BatchMPC
    return BatchMPC(N=N, dtype=torch.float32 if f32 else torch.float64, model=model, weights=weights, **kw)


def _solve(s, d, params=None):
    import torch
    fn = s.solve_frenet if s.cfg.model == 1 else s.solve
    o = fn(d["z0"], d["second"], d["v_target"], d["u_prev"], want_U=True, want_X=True, params=params)
    torch.cuda.synchronize()
    return {k: o[k].cpu().numpy() for k in KEYS}


def _same(a, b, rows, what):
    for k in KEYS:
        x, y = a[k][rows], b[k][rows]
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), \
            "%s: %s differs on %d of %d rows" % (what, k, int((x != y).reshape(len(x), -1).any(1).sum()), len(x))


# (what, model, N, B, fp32, options): every back-end in fp64; the fp32 instantiations of the quad, one-wave and four-wave kernels
BACKENDS = [("one-wave N=8", 0, 8, 512, False, dict(kernel_variant=2)), ("one-wave N=12", 0, 12, 512, False, {}), ("one-wave N=20", 0, 20, 1024, False, {}),
            ("one-wave N=28", 0, 28, 256, False, {}), ("dense N=12", 0, 12, 4096, False, dict(kernel_variant=2)), ("four-wave N=32", 0, 32, 256, False, {}),
            ("four-wave N=50", 0, 50, 256, False, {}), ("quad N=8", 0, 8, 4096, False, {}), ("generic N=10", 0, 10, 256, False, {}),
            ("Frenet one-wave N=8", 1, 8, 512, False, {}), ("Frenet one-wave N=20", 1, 20, 256, False, {}), ("Frenet four-wave N=40", 1, 40, 64, False, {}),
            ("Frenet generic N=10", 1, 10, 128, False, {}), ("Frenet quad N=8", 1, 8, 512, False, dict(kernel_variant=3)),
            ("quad N=8 fp32", 0, 8, 4096, True, {}), ("one-wave N=20 fp32", 0, 20, 1024, True, {}), ("four-wave N=50 fp32", 0, 50, 256, True, {})]


@pytest.mark.gpu
@pytest.mark.parametrize("what,model,N,B,f32,kw", BACKENDS, ids=[b[0].replace(" ", "-") for b in BACKENDS])
def test_params_equal_per_set_handles_bit_for_bit(what, model, N, B, f32, kw):
    """2: same kernel, same answer.  The per-set call runs the full batch on a handle that carries the set (problems of other sets may be infeasible under it:
    their rows are not compared), so dispatch thresholds and the start-order pre-pass see the same batch in both calls."""
    d, sets, rec = _draw(N, B, model, np.float32 if f32 else np.float64)
    s = _mpc(N, f32, model, **kw)
    a = _solve(s, d, params=rec)
    s.close()
    n_opt = int((a["status"] == 0).sum())
    print("%s: through params: status %s, iters mean %.2f max %d" % (what, np.bincount(a["status"], minlength=4).tolist(), a["iters"].mean(), a["iters"].max()))
    assert np.isfinite(a["U"]).all() and np.isfinite(a["cost"]).all()
    if not f32:
        assert n_opt == B, what   # (the CPU port is all-Optimal on these draws; fp32 ends a few problems at its rounding floor as on the default weights)
    for g, (w, lim) in enumerate(sets):
        h = _mpc(N, f32, model, weights=list(w), **dict(kw, **lim))
        b = _solve(h, d)
        h.close()
        _same(a, b, np.arange(g, B, G), "%s set %d" % (what, g))


@pytest.mark.gpu
@pytest.mark.parametrize("what,model,N,B,f32,kw", [b for b in BACKENDS if not b[4]], ids=[b[0].replace(" ", "-") for b in BACKENDS if not b[4]])
def test_handle_values_through_params_is_the_plain_call(what, model, N, B, f32, kw):
    """3: problem_params(B) carries the handle's own values: the new path gives the plain call's bits"""
    d, _, _ = _draw(N, B, model)
    s = _mpc(N, f32, model, **kw)
    rec = s.problem_params(B)
    assert tuple(rec.shape) == (B, 16) and rec.dtype == s.dtype and rec.device == s.device
    w = (C.c_double * 8)()
    s.lib.kmpc_get_cost(s.h, w)
    row = rec[0].cpu().numpy()
    assert np.array_equal(row[:8], np.array(w[:])) and row[13] == s.cfg.v_max and row[8] == s.cfg.steer_max and (row[14:] == 0).all()
    _same(_solve(s, d, params=rec), _solve(s, d), np.arange(B), what)
    s.close()


# every compiled instantiation of the parameter kernels: (model, N, B, fp32, options).  Several of them carry scratch where their plain twin has none or less
# (tools/kernel_resources.py; DESIGN.md section 9 wants every instantiation with scratch checked independently): here each one must reproduce, bit for bit, the
# plain kernel of the same horizon, model and precision -- which tests/test_certify.py certifies -- on a seeded batch
ALL_INSTANTIATIONS = [(0, N, 256, f32, dict(kernel_variant=2)) for N in (8, 12, 16, 20, 24, 28) for f32 in (False, True)]
ALL_INSTANTIATIONS += [(0, N, 2304, f32, dict(kernel_variant=2)) for N in (8, 12) for f32 in (False, True)]            # the denser build (B > 2048)
ALL_INSTANTIATIONS += [(0, N, 64, f32, {}) for N in (32, 36, 40, 44, 48, 50) for f32 in (False, True)]
ALL_INSTANTIATIONS += [(0, 8, 1024, f32, {}) for f32 in (False, True)]                                                   # four per wave
ALL_INSTANTIATIONS += [(1, N, 256, f32, {}) for N in (8, 12, 16, 20, 24, 28) for f32 in (False, True)]
ALL_INSTANTIATIONS += [(1, N, 64, False, {}) for N in (32, 36, 40, 44, 48, 50)]
ALL_INSTANTIATIONS += [(1, 8, 512, f32, dict(kernel_variant=3)) for f32 in (False, True)]
ALL_INSTANTIATIONS += [(0, N, 64, f32, dict(kernel_variant=1)) for N in (6, 14, 22, 30, 38, 46, 54) for f32 in (False, True)]   # generic kernel, NT = 1 ... 7
ALL_INSTANTIATIONS += [(1, N, 64, f32, dict(kernel_variant=1)) for N in (6, 14, 22) for f32 in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("model,N,B,f32,kw", ALL_INSTANTIATIONS,
                         ids=["%s-N%d-B%d-%s-v%d" % ("frenet" if m else "cart", N, B, "f32" if f else "f64", kw.get("kernel_variant", 0)) for m, N, B, f, kw in ALL_INSTANTIATIONS])
def test_every_parameter_instantiation_reproduces_its_plain_kernel(model, N, B, f32, kw):
    if model == 0:
        b = make_batch(B, N, cfg_id=2, seed=5300 + N)
        d = dict(z0=b["z0"], second=b["ref"], v_target=b["v_target"], u_prev=b["u_prev"])
    elif N <= 28:
        z0, kp, vt, up = _cases(B, N, seed=900 + N)
        d = dict(z0=z0, second=kp, v_target=vt, u_prev=up)
    else:
        from test_frenet_wide import _long_cases
        z0, kp, vt, up = _long_cases(B, N, seed=900 + N)
        d = dict(z0=z0, second=kp, v_target=vt, u_prev=up)
    d = {k: np.ascontiguousarray(v, dtype=np.float32 if f32 else np.float64) for k, v in d.items()}
    s = _mpc(N, f32, model, **kw)
    a, b = _solve(s, d, params=s.problem_params(B)), _solve(s, d)
    s.close()
    assert (b["status"] == 0).sum() >= B // 2, np.bincount(b["status"])   # (a real solve on both sides, not two early exits)
    _same(a, b, np.arange(B), "model %d N=%d %s" % (model, N, "fp32" if f32 else "fp64"))


@pytest.mark.gpu
def test_params_none_goes_through_the_old_symbol(monkeypatch):
    d, _, rec = _draw(8, 64)
    s = _mpc(8, kernel_variant=2)
    calls = []

    class Spy:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            f = getattr(self._lib, name)
            if name.startswith("kmpc_solve_batch"):
                def g(*a):
                    calls.append(name)
                    return f(*a)
                return g
            return f
    s.lib = Spy(s.lib)
    _solve(s, d)
    _solve(s, d, params=None)
    assert calls == ["kmpc_solve_batch", "kmpc_solve_batch"]
    _solve(s, d, params=rec)
    assert calls[-1] == "kmpc_solve_batch_params"
    with pytest.raises(ValueError):
        _solve(s, d, params=rec[:, :15])
    s.lib = s.lib._lib
    # the C entry point itself: params == NULL is exactly the plain call
    import torch
    dev = {k: torch.as_tensor(v, device=s.device) for k, v in d.items()}
    u0a, u0b = torch.empty((64, 2), dtype=s.dtype, device=s.device), torch.empty((64, 2), dtype=s.dtype, device=s.device)
    sta, stb = torch.empty(64, dtype=torch.int32, device=s.device), torch.empty(64, dtype=torch.int32, device=s.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert s.lib.kmpc_solve_batch_params(s.h, 64, p(dev["z0"]), p(dev["second"]), p(dev["v_target"]), p(dev["u_prev"]), None, None, 0, p(u0a), p(sta), None, None, None,
                                         None, None, None) == 0
    assert s.lib.kmpc_solve_batch(s.h, 64, p(dev["z0"]), p(dev["second"]), p(dev["v_target"]), p(dev["u_prev"]), None, 0, p(u0b), p(stb), None, None, None, None, None,
                                  None) == 0
    torch.cuda.synchronize()
    assert torch.equal(u0a, u0b) and torch.equal(sta, stb)
    # a Frenet handle refuses the Cartesian entry point and vice versa
    assert s.lib.kmpc_solve_batch_frenet_params(s.h, 64, p(dev["z0"]), p(dev["second"]), p(dev["v_target"]), p(dev["u_prev"]), p(dev["z0"]), None, 0, p(u0a), p(sta),
                                                None, None, None, None, None, None) != 0
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N,B,strict", [(8, 1024, 1e-6), (20, 1024, 1e-6), (50, 256, 2e-6)])
def test_solutions_certify_under_their_own_parameters(oracle, N, B, strict):
    """4: N = 8 runs the four-per-wave kernel (B >= 1024, its per-row parameter tables), N = 20 the one-wave, N = 50 the four-wave kernel"""
    from test_certify import _assert_certified
    O = oracle
    d, sets, rec = _draw(N, B)
    s = _mpc(N)
    r = _solve(s, d, params=rec)
    relax = s.cfg.bound_relax
    s.close()
    assert (r["status"] == 0).all(), np.bincount(r["status"])
    dd = dict(z0=d["z0"], ref=d["second"], v_target=d["v_target"], u_prev=d["u_prev"])
    for g, (w, lim) in enumerate(sets):
        idx = np.arange(g, B, G)
        assert len(idx) < 256   # (the pooled path of certify_batch rebuilds the parameters without the limits)
        c = CT.certify_batch(O, O.params(N, list(w), **lim), dd, r["U"], idx=idx)
        _assert_certified(c, strict, relax * max(1.0, lim["v_max"]) + 1e-12, "N = %d set %d" % (N, g))
        assert np.abs(c["cost"] - r["cost"][idx]).max() <= 1e-9 * max(1.0, np.abs(r["cost"][idx]).max())   # reported cost = the objective under the set's weights


@pytest.mark.gpu
@pytest.mark.parametrize("what,N,B,kw", [("one-wave", 20, 256, {}), ("quad", 8, 1024, {}), ("four-wave", 32, 64, {}), ("generic", 10, 64, {})])
def test_bad_and_infeasible_records(what, N, B, kw):
    """5"""
    d, sets, rec = _draw(N, B)
    s = _mpc(N, **kw)
    good = _solve(s, d, params=rec)
    bad = rec.copy()
    fast = np.where(d["z0"][:, 3] > 2.0)[0]
    i_nan, i_neg, i_v, i_res, i_inf = 5, B // 4 + 6, B // 2 + 3, B - 1, int(fast[len(fast) // 2])
    assert len({i_nan, i_neg, i_v, i_res, i_inf}) == 5
    bad[i_nan, 2] = np.nan
    bad[i_neg, 6] = -1.0
    bad[i_v, 13] = bad[i_v, 12]
    bad[i_res, 15] = 1.0
    bad[i_inf, 13] = d["z0"][i_inf, 3] - 1.0
    r = _solve(s, d, params=bad)
    for i in (i_nan, i_neg, i_v, i_res):
        assert r["status"][i] == 3 and r["iters"][i] == 0 and r["cost"][i] == 0 and r["viol"][i] == 0, (what, i, r["status"][i], r["iters"][i])
        assert (r["u0"][i] == 0).all() and (r["U"][i] == 0).all() and (r["X"][i] == 0).all()
    # the infeasible one: what a handle with that v_max reports for the same problem
    w, lim = sets[i_inf % G]
    h = _mpc(N, weights=list(w), **dict(kw, **dict(lim, v_max=float(bad[i_inf, 13]))))
    ref = _solve(h, d)
    h.close()
    assert ref["status"][i_inf] == 2
    _same(r, ref, np.array([i_inf]), what + " infeasible record")
    others = np.setdiff1d(np.arange(B), [i_nan, i_neg, i_v, i_res, i_inf])
    _same(r, good, others, what + " other problems")
    s.close()


@pytest.mark.gpu
def test_limits_bite():
    """6: N = 20, batch seed 5120, sets from seed 5121.  Set 3 (v_max = 9.81) has 26 problems with v_target above its limit; on the CPU port 27 problems of the set
    end with the speed row active and none of any other set."""
    N, B = 20, 1024
    d, sets, rec = _draw(N, B)
    s = _mpc(N)
    r = _solve(s, d, params=rec)
    relax = s.cfg.bound_relax
    s.close()
    assert (r["status"] == 0).all()
    vmax = rec[:, 13]
    top = r["X"][:, :, 3].max(1)
    assert (top <= vmax + relax * np.maximum(1.0, vmax) + 1e-12).all(), float((top - vmax).max())
    active = top >= vmax - 1e-3
    per_set = [int(active[g::G].sum()) for g in range(G)]
    w, lim = sets[3]
    h = _mpc(N, weights=list(w), **dict(lim, v_max=20.0))
    free = _solve(h, d)
    h.close()
    rows = np.arange(3, B, G)
    over = int((free["X"][rows, :, 3].max(1) > lim["v_max"] + 1e-3).sum())
    print("speed row active per set: %s; set 3 problems above %.3f m/s under v_max = 20: %d" % (per_set, lim["v_max"], over))
    assert per_set[3] >= 20 and over >= 20, (per_set, over)


@pytest.mark.gpu
def test_mixed_fleet_closed_loop():
    """7: 64 vehicles on the path-3 fixture in target-velocity mode, two parameter sets alternating, 50 control periods, against two homogeneous loops whose handles
    carry the sets (same starts): state and command histories are bit-identical vehicle by vehicle (test 2 is bit-identical for this kernel)."""
    import torch
    import scenario as S
    from mkz_mpc_path_follower_amd.ref_traj import GPSRefTrajectory
    from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator
    from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop
    L = S.LAUNCH
    arr, lat0, lon0 = S.path_arrays()
    B, steps, tv = 64, 50, 5.0
    rng = np.random.default_rng(3)
    X0, Y0, P0 = L["X0"] + rng.uniform(-2, 2, B), L["Y0"] + rng.uniform(-2, 2, B), L["Psi0"] + rng.uniform(-0.5, 0.5, B)
    sets = make_param_sets(2, 7000)

    def run(params_of, **mpc_kw):
        grt = GPSRefTrajectory(arrays=arr, traj_horizon=8, traj_dt=0.2, lat0=lat0, lon0=lon0)
        sim = VehicleSimulator(B, X0=X0, Y0=Y0, Psi0=P0)
        loop = ClosedLoop(grt, sim, N=8, target_vel=tv, track_with_time=False, kernel_variant=2, **mpc_kw)
        if params_of is not None:
            loop.params = params_of(loop.mpc)
        st, cmd, status = [sim.state.cpu().numpy().copy()], [], []
        for _ in range(steps):
            o = loop.step()
            torch.cuda.synchronize()
            st.append(sim.state.cpu().numpy().copy()); cmd.append(o["cmd"].cpu().numpy().copy()); status.append(o["status"].cpu().numpy().copy())
        loop.mpc.close()
        return np.array(st), np.array(cmd), np.array(status)

    def mixed(mpc):
        p = mpc.problem_params(B)
        p.copy_(torch.as_tensor(param_records(sets, B), device=p.device))
        return p
    st, cmd, status = run(mixed)
    assert (status == 0).all(), np.bincount(status.ravel())
    for g, (w, lim) in enumerate(sets):
        sg, cg, _ = run(None, weights=tuple(w), **lim)
        assert np.array_equal(st[:, g::2], sg[:, g::2]) and np.array_equal(cmd[:, g::2], cg[:, g::2]), \
            (g, float(np.abs(st[:, g::2] - sg[:, g::2]).max()), float(np.abs(cmd[:, g::2] - cg[:, g::2]).max()))
        assert np.abs(cmd[:, 1 - g::2] - cg[:, 1 - g::2]).max() > 1e-3   # (the other set's vehicles drive differently under this set: the records are what is honoured)
    assert not np.array_equal(st[:, 0], st[:, 1])
