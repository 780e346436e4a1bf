"""Four Frenet problems per wave at the Frenet reference's own horizon N = 8 (csrc/kmpc_quad.hip, kmpc_solve_quad_frenet_kernel;
MKZMPCPathFollowerFrenet.jl:33): one problem per 16-lane DPP row, reached through kmpc_solve_batch_frenet with kmpc_config.kernel_variant = 3
(model 1, N = 8 only).  kernel_variant 2 is the one-wave-per-problem Frenet kernel it is compared with; the default dispatch is unchanged.

CPU part: static resources of the new kernel.  GPU part: handles, parity with the oracle and with the one-wave kernel, certification, row
independence / determinism / containment, options, warm start, the slack guard, the module API and the fp32 acceptance."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from test_frenet import _cases  # noqa: E402

N = 8
KEYS = ("U", "X", "cost", "viol", "iters", "status", "u0")
# kmpc_solve_quad_frenet_kernel<double>, as the committed source compiles: LDS bytes (four rows of 740 words + parameter and coefficient tables), waves per
# CU (by LDS: 160 KiB / 24 192 B = 6; the 256 VGPRs alone would allow 8) and scratch bytes (the Cartesian quad kernel carries 60)
QUAD_FRENET_RESOURCES = dict(lds=24192, waves_per_cu=6, scratch=68)


# ------------------------------------------------------------------------------------------------ CPU
def test_frenet_quad_kernel_static_resources():
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import static_mix as M
    rows = {r["kernel"]: r for r in M.analyse(os.path.join(ROOT, "mkz_mpc_path_follower_amd", "csrc", "kmpc_quad.hip"), ["kmpc_solve_quad_frenet_kernel"])}
    r = rows["kmpc_solve_quad_frenet_kernel<double>"]
    assert r["lds"] == QUAD_FRENET_RESOURCES["lds"], r
    assert r["vgprs"] <= 256, r                                   # two waves per SIMD by registers
    assert r["waves_per_cu"] == QUAD_FRENET_RESOURCES["waves_per_cu"], r
    assert r["scratch"] == QUAD_FRENET_RESOURCES["scratch"], r    # pinned: growth must be seen (and certified)
    assert "kmpc_solve_quad_frenet_kernel<float>" in rows         # fp32: accepted (test_frenet_quad_fp32_acceptance)


# ------------------------------------------------------------------------------------------------ GPU
def _solve(z0, kp, vt, up, dtype=None, **kw):
    import torch
    from mkz_mpc_path_follower_amd import BatchMPC
    warm_U = kw.pop("warm_U", None)
    kw.setdefault("kernel_variant", 3)
    s = BatchMPC(N=N, dtype=dtype or torch.float64, model=1, **kw)
    o = s.solve_frenet(z0, kp, vt, up, warm_U=warm_U, warm=warm_U is not None, want_U=True, want_X=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


@pytest.mark.gpu
def test_frenet_quad_handles():
    import torch
    from mkz_mpc_path_follower_amd import BatchMPC, _lib
    BatchMPC(N=8, dtype=torch.float64, model=1, kernel_variant=3).close()
    with pytest.raises(_lib.KmpcError, match="model = 1"):
        BatchMPC(N=8, dtype=torch.float64, model=0, kernel_variant=3)
    for n in (12, 32):
        with pytest.raises(_lib.KmpcError, match="N = 8"):
            BatchMPC(N=n, dtype=torch.float64, model=1, kernel_variant=3)
    BatchMPC(N=8, dtype=torch.float32, model=1, kernel_variant=3).close()   # fp32: accepted (test_frenet_quad_fp32_acceptance)
    for kv in (0, 1, 2):   # unchanged
        BatchMPC(N=8, dtype=torch.float64, model=1, kernel_variant=kv).close()
    with pytest.raises(_lib.KmpcError):
        BatchMPC(N=8, dtype=torch.float64, model=1, kernel_variant=4)


@pytest.mark.gpu
@pytest.mark.parametrize("B,seed", [(1024, 31), (4099, 32), (8192, 33)])
def test_frenet_quad_matches_oracle_and_one_wave_kernel(oracle, B, seed):
    """batch sizes incl. one that is not a multiple of four; against the oracle the tolerances of test_frenet_kernel_matches_oracle, against the
    one-wave kernel those of test_frenet_compile_time_and_generic_kernels_agree"""
    O = oracle
    z0, kp, vt, up = _cases(B, N, seed)
    g = _solve(z0, kp, vt, up)
    w = _solve(z0, kp, vt, up, kernel_variant=2)
    r = O.solve_condensed_batch(O.params(N, model=1), z0, kp, vt, up, nthreads=8, want_X=True)
    assert (g["status"] == 0).all() and (r["status"] == 0).all(), (np.bincount(g["status"]), np.bincount(r["status"]))
    print("oracle: cost %.2e viol %.2e u0 %.2e X %.2e iters %.3f / %.3f" % (
        _rel(g["cost"], r["cost"]).max(), g["viol"].max(), np.abs(g["u0"] - r["U"].reshape(B, N, 2)[:, 0, :]).max(), np.abs(g["X"] - r["X"]).max(),
        g["iters"].mean(), r["iters"].mean()))
    assert _rel(g["cost"], r["cost"]).max() <= 1e-6
    assert g["viol"].max() <= 1e-8 + 1e-12
    assert np.abs(g["u0"] - r["U"].reshape(B, N, 2)[:, 0, :]).max() <= 1e-6
    assert np.abs(g["X"] - r["X"]).max() <= 1e-5
    assert abs(g["iters"].mean() - r["iters"].mean()) < 1.0
    print("one-wave: cost %.2e X %.2e iters %.3f / %.3f" % (_rel(g["cost"], w["cost"]).max(), np.abs(g["X"] - w["X"]).max(), g["iters"].mean(), w["iters"].mean()))
    assert np.array_equal(g["status"], w["status"])
    assert _rel(g["cost"], w["cost"]).max() <= 1e-7 and abs(g["iters"].mean() - w["iters"].mean()) < 0.5
    assert np.abs(g["X"] - w["X"]).max() <= 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2, 3, 5])
def test_frenet_quad_partial_waves(B):
    """a wave with one to three live rows (the others repeat the last problem) returns what the one-wave kernel returns"""
    z0, kp, vt, up = (a[:B] for a in _cases(5, N, 37))
    g = _solve(z0, kp, vt, up)
    w = _solve(z0, kp, vt, up, kernel_variant=2)
    assert (w["status"] == 0).all() and np.array_equal(g["status"], w["status"])
    assert _rel(g["cost"], w["cost"]).max() <= 1e-7 and abs(g["iters"].mean() - w["iters"].mean()) < 0.5
    assert np.abs(g["X"] - w["X"]).max() <= 1e-6


@pytest.mark.gpu
def test_frenet_quad_certified(oracle):
    """every returned U is a KKT point of the Frenet NLP: the loop and the bounds of test_certify.py::test_certify_frenet_functor"""
    import certify as CT
    from test_certify import _assert_certified
    O = oracle
    B = 1024
    z0, kp, vt, up = _cases(B, N, 33)
    g = _solve(z0, kp, vt, up)
    assert (g["status"] == 0).all(), np.bincount(g["status"])
    p = O.params(N, model=1)
    out = {k: [] for k in CT.KEYS}
    for b in range(B):
        c = CT.certify_problem(O, p, O.problem_frenet(p, z0[b], kp[b], vt[b], up[b]), g["U"][b])
        for k in CT.KEYS:
            out[k].append(c[k])
    _assert_certified({k: np.array(v) for k, v in out.items()}, 1e-6, 1e-8 + 1e-12, "quad Frenet N=8")


@pytest.mark.gpu
def test_frenet_quad_row_independence_determinism_containment():
    B = 512
    z0, kp, vt, up = _cases(B, N, 35)
    a = _solve(z0, kp, vt, up)
    b = _solve(z0, kp, vt, up)
    assert (a["status"] == 0).all()
    for k in KEYS:   # two runs of the same batch
        assert np.array_equal(a[k], b[k]), k
    # a problem's result does not depend on its row or its neighbours: alone (row 0, three copies beside it) and in a permuted batch
    for i in (0, 5, 11, 254, 511):
        one = _solve(z0[i:i + 1], kp[i:i + 1], vt[i:i + 1], up[i:i + 1])
        assert one["status"][0] == a["status"][i] and one["iters"][0] == a["iters"][i], i
        assert _rel(one["cost"][0], a["cost"][i]) <= 1e-9, i
    perm = np.random.default_rng(0).permutation(B)
    c = _solve(z0[perm], kp[perm], vt[perm], up[perm])
    assert np.array_equal(c["status"], a["status"][perm]) and np.array_equal(c["iters"], a["iters"][perm])
    assert _rel(c["cost"], a["cost"][perm]).max() <= 1e-9
    for k in KEYS:   # (more than asked: a row's arithmetic does not depend on its position in the wave, so the bits are the same too)
        assert np.array_equal(c[k], a[k][perm]), k
    # a NaN in one problem's k_poly: that problem fails, the three other rows of its wave and everything else are bit-equal to the clean run
    kp2 = kp.copy()
    kp2[5, 1] = np.nan
    d = _solve(z0, kp2, vt, up)
    assert d["status"][5] != 0
    rest = np.arange(B) != 5
    for k in KEYS:
        assert np.array_equal(d[k][rest], a[k][rest]), k


@pytest.mark.gpu
@pytest.mark.parametrize("opts", [dict(), dict(indef_strategy=0), dict(indef_strategy=1), dict(hessian=0), dict(start=1),
                                  dict(weights=(0.0, 20.0, 5.0, 1.0, 50.0, 500.0, 0.1, 0.1))])
def test_frenet_quad_options(opts):
    """same statuses as the one-wave kernel with the same options, costs to 1e-7 on the problems Optimal in both; the default options: all Optimal"""
    z0, kp, vt, up = _cases(512, N, 35)
    g = _solve(z0, kp, vt, up, **opts)
    w = _solve(z0, kp, vt, up, kernel_variant=2, **opts)
    print(opts, np.bincount(g["status"], minlength=4), np.bincount(w["status"], minlength=4))
    assert np.array_equal(g["status"], w["status"]), opts
    ok = (g["status"] == 0) & (w["status"] == 0)
    assert not ok.any() or _rel(g["cost"], w["cost"])[ok].max() <= 1e-7, opts
    if not opts:
        assert ok.all()


@pytest.mark.gpu
def test_frenet_quad_warm_start():
    z0, kp, vt, up = _cases(512, N, 35)
    cold = _solve(z0, kp, vt, up)
    warm = _solve(z0, kp, vt, up, warm_U=cold["U"])
    warm1 = _solve(z0, kp, vt, up, warm_U=cold["U"], kernel_variant=2)   # the one-wave kernel on the same warm start
    assert (cold["status"] == 0).all() and (warm["status"] == 0).all() and (warm1["status"] == 0).all()
    print("warm iterations: quad %.3f one-wave %.3f cold %.3f" % (warm["iters"].mean(), warm1["iters"].mean(), cold["iters"].mean()))
    assert abs(warm["iters"].mean() - warm1["iters"].mean()) <= 0.5


@pytest.mark.gpu
def test_slack_guard_trips_in_the_frenet_quad_kernel():
    """the run-time slack guard of ipm::solve in the new kernel: with the TEST build libkmpc_hip_corrupt.so no solve may end Optimal (child process)"""
    lib = os.path.join(ROOT, "mkz_mpc_path_follower_amd", "libkmpc_hip_corrupt.so")
    assert os.path.exists(lib), "build it: make -C mkz_mpc_path_follower_amd/csrc (the default target builds it)"
    r = subprocess.run([sys.executable, os.path.join(HERE, "_corrupt_probe_frenet_quad.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("CORRUPT_PROBE ")][-1]
    n_opt, n_lim, n_inf, n_err = json.loads(line[len("CORRUPT_PROBE "):])["quad_frenet_f64_N8"]
    assert n_opt == 0 and n_err > 0, (n_opt, n_lim, n_inf, n_err)


@pytest.mark.gpu
def test_frenet_quad_module_api(oracle):
    """the checks of test_frenet.py::test_frenet_module_api with KinematicMPCFrenet(kernel_variant=3): B = 1, three rows of the wave repeat the problem"""
    from mkz_mpc_path_follower_amd.kinematic_mpc_frenet import KinematicMPCFrenet
    O = oracle
    m = KinematicMPCFrenet(N=8, kernel_variant=3)
    assert m.status == "Optimal"
    s_, ey_, v_, epsi_, K_, path_, df_, acc_ = m.get_solver_results()
    assert abs(acc_[0] - 0.15) < 1e-6 and np.abs(df_).max() < 1e-7 and np.abs(ey_).max() < 1e-9
    m.update_init_cond(1.5, 0.4, -0.05, 6.0)
    m.update_reference({"x": [0.0], "y": [0.0]}, [1e-5, -2e-4, 1e-3, 0.03], 7.0)
    m.update_current_input(0.01, 0.2)                 # steer first
    m.update_cost(9.0, 10.0, 0.5, 100.0, 1000.0, 0.0, 0.0)
    a, d, st = m.solve_model()
    assert st == "Optimal"
    p = O.params(8, model=1)
    r = O.solve_condensed(p, O.problem_frenet(p, [1.5, 0.4, -0.05, 6.0], [1e-5, -2e-4, 1e-3, 0.03], 7.0, (0.2, 0.01)))
    assert abs(m.cost - r["cost"]) <= 1e-6 * max(1.0, r["cost"]) and abs(a - r["U"][0, 0]) < 1e-6 and abs(d - r["U"][0, 1]) < 1e-6
    res = m.get_solver_results()
    assert np.allclose(res[0], r["X"][:, 0], atol=1e-6) and np.allclose(res[2], r["X"][:, 3], atol=1e-6)
    assert np.allclose(res[3], r["X"][:, 2], atol=1e-6) and res[5] == {"x": [0.0], "y": [0.0]}
    a2, d2, st2 = m.solve_model()                     # warm re-solve of the same problem
    assert st2 == "Optimal" and abs(a2 - a) < 1e-6


@pytest.mark.gpu
def test_frenet_quad_fp32_acceptance():
    """what decided that kernel_variant = 3 accepts KMPC_F32.  Yardstick: the one-wave fp32 Frenet kernel on the same draw -- the new kernel may leave
    at most as many problems non-Optimal; for its Optimal problems the bounds test_quad_fp32_and_warm_start holds the Cartesian fp32 quad kernel
    to against its fp64 self (violation <= 1e-4, 99th percentile of the relative cost difference <= 1e-3), and none may differ from the fp64 cost by
    more than 1e-2 relative (the fp32 certificate bound of test_certify.py as the false-Optimal line).
    Measured on (4099, seed 32): see DESIGN.md section 4d."""
    import torch
    z0, kp, vt, up = _cases(4099, N, 32)
    q64 = _solve(z0, kp, vt, up)
    q32 = _solve(z0, kp, vt, up, dtype=torch.float32)
    w32 = _solve(z0, kp, vt, up, dtype=torch.float32, kernel_variant=2)
    assert (q64["status"] == 0).all()
    bad_q, bad_w = int((q32["status"] != 0).sum()), int((w32["status"] != 0).sum())
    ok = q32["status"] == 0
    rel = _rel(q32["cost"].astype(np.float64), q64["cost"])
    print("fp32 non-Optimal: quad %d one-wave %d of 4099; Optimal: viol max %.2e, rel cost p99 %.2e max %.2e" % (
        bad_q, bad_w, q32["viol"][ok].max(), np.percentile(rel[ok], 99), rel[ok].max()))
    assert bad_q <= bad_w, (bad_q, bad_w)
    assert q32["viol"][ok].max() <= 1e-4
    assert np.percentile(rel[ok], 99) <= 1e-3
    assert rel[ok].max() <= 1e-2
