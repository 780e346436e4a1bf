"""The Frenet-frame functor (MKZMPCPathFollowerFrenet.jl, cfg.model = 1) in the four-wave kernel (kmpc_wide.hip, N = 32 ... 48 and 50, fp64).

CPU part: the oracle on the long-horizon case generator, static resources of the new kernel.  GPU part: handle creation, parity with the
oracle, certification, Hessian strategies, warm start, the module API, containment / determinism and the run-time slack guard."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WIDE_N = (32, 36, 40, 44, 48, 50)


def _long_cases(B, N, seed=3):
    """as test_frenet._cases, but the curvature polynomial is scaled to x = s / 200 m: over 50 stages at up to ~15 m/s the vehicle travels
    ~150 m, and the 60 m scaling of the short-horizon generator then runs into |K| up to 0.74 1/m (and problems the oracle fails too)"""
    rng = np.random.default_rng(seed)
    z0 = np.stack([rng.uniform(0, 5, B), rng.normal(0, 0.4, B), rng.normal(0, 0.08, B), rng.uniform(2, 12, B)], 1)
    a, b, c, d = rng.uniform(-0.04, 0.04, B), rng.normal(0, 0.015, B), rng.normal(0, 0.015, B), rng.normal(0, 0.015, B)
    kp = np.stack([d / 200.0 ** 3, c / 200.0 ** 2, b / 200.0, a], 1)  # highest degree first
    vt = np.clip(z0[:, 3] + rng.normal(0, 1.0, B), 1.0, 15.0)
    up = np.stack([rng.uniform(-0.4, 0.4, B), rng.uniform(-0.05, 0.05, B)], 1)
    return z0, kp, vt, up


def _curvature(kp, s):
    return ((kp[:, 0:1] * s + kp[:, 1:2]) * s + kp[:, 2:3]) * s + kp[:, 3:4]


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("N", [32, 50])
def test_long_cases_are_road_like_and_solvable(oracle, N):
    O = oracle
    z0, kp, vt, up = _long_cases(400, N)
    r = O.solve_condensed_batch(O.params(N, model=1), z0, kp, vt, up, nthreads=8, want_X=True)
    assert (r["status"] == 0).all(), np.bincount(r["status"])
    assert np.abs(_curvature(kp, r["X"][:, :, 0])).max() <= 0.1


# kmpc_solve_wide_frenet_kernel<double, N>: LDS bytes and what tools/static_mix.py reports as waves per CU.  Every instantiation holds 245-256 VGPRs:
# two workgroups (of four waves) per CU at every N; the tool's figure for N = 32 / 36 is the LDS bound alone (three workgroups' worth of LDS).
FRENET_WIDE_RESOURCES = {32: (46688, 3), 36: (52544, 3), 40: (59936, 2), 44: (66816, 2), 48: (75232, 2), 50: (79120, 2)}


@pytest.fixture(scope="module")
def wide_rows():
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import static_mix as M
    return {r["kernel"]: r for r in M.analyse(os.path.join(ROOT, "mkz_mpc_path_follower_amd", "csrc", "kmpc_wide.hip"), ["kmpc_solve_wide_frenet_kernel"])}


@pytest.mark.parametrize("N", WIDE_N)
def test_frenet_wide_kernel_static_resources(wide_rows, N):
    r = wide_rows["kmpc_solve_wide_frenet_kernel<double, %d>" % N]
    lds, wpc = FRENET_WIDE_RESOURCES[N]
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
    assert r["lds"] == lds and r["lds"] <= 81920, r           # two workgroups per CU by LDS
    assert r["vgprs"] <= 256, r                               # two waves per SIMD = two workgroups per CU by registers
    assert r["waves_per_cu"] == wpc, r
    assert not any("kmpc_solve_wide_frenet_kernel<float" in k for k in wide_rows)   # fp32: refused by kmpc_create, not compiled


# ------------------------------------------------------------------------------------------------ GPU
def _solve(N, z0, kp, vt, up, **kw):
    import torch
    from mkz_mpc_path_follower_amd import BatchMPC
    warm_U = kw.pop("warm_U", None)
    s = BatchMPC(N=N, dtype=torch.float64, model=1, **kw)
    o = s.solve_frenet(z0, kp, vt, up, warm_U=warm_U, warm=warm_U is not None, want_U=True, want_X=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


@pytest.mark.gpu
def test_frenet_wide_handles():
    import torch
    from mkz_mpc_path_follower_amd import BatchMPC, _lib
    for N in WIDE_N:
        for kv in (0, 2):
            BatchMPC(N=N, dtype=torch.float64, model=1, kernel_variant=kv).close()
    with pytest.raises(_lib.KmpcError):
        BatchMPC(N=32, dtype=torch.float64, model=1, kernel_variant=1)
    with pytest.raises(_lib.KmpcError):
        BatchMPC(N=30, dtype=torch.float64, model=1)
    for N in WIDE_N:   # fp32 four-wave Frenet: not shipped
        with pytest.raises(_lib.KmpcError, match="fp64 only"):
            BatchMPC(N=N, dtype=torch.float32, model=1)
    BatchMPC(N=28, dtype=torch.float32, model=1).close()   # (unchanged below)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [32, 40, 50])
def test_frenet_wide_matches_oracle(oracle, N):
    """the tolerances of test_frenet.py::test_frenet_kernel_matches_oracle, predicted states scaled for up to 50 stages"""
    O = oracle
    B = 512
    z0, kp, vt, up = _long_cases(B, N, seed=21)
    g = _solve(N, z0, kp, vt, up)
    r = O.solve_condensed_batch(O.params(N, model=1), z0, kp, vt, up, nthreads=8, want_X=True)
    assert (g["status"] == 0).all() and (r["status"] == 0).all(), (np.bincount(g["status"]), np.bincount(r["status"]))
    rel = np.abs(g["cost"] - r["cost"]) / np.maximum(1.0, np.abs(r["cost"]))
    assert rel.max() <= 1e-6
    assert g["viol"].max() <= 1e-8 + 1e-12
    assert np.abs(g["u0"] - r["U"].reshape(B, N, 2)[:, 0, :]).max() <= 1e-6
    assert np.abs(g["X"] - r["X"]).max() <= 2e-5
    assert abs(g["iters"].mean() - r["iters"].mean()) < 1.0


@pytest.mark.gpu
def test_frenet_wide_certified(oracle):
    """every returned U of a B = 1024 batch at N = 50 is a KKT point of the Frenet NLP (NNLS multipliers from U alone, tests/certify.py)"""
    from concurrent.futures import ThreadPoolExecutor
    sys.path.insert(0, HERE)
    import certify as CT
    from test_certify import _assert_certified
    O = oracle
    N, B = 50, 1024
    z0, kp, vt, up = _long_cases(B, N, seed=41)
    g = _solve(N, z0, kp, vt, up)
    assert (g["status"] == 0).all(), np.bincount(g["status"])
    p = O.params(N, model=1)

    def one(b):
        return CT.certify_problem(O, p, O.problem_frenet(p, z0[b], kp[b], vt[b], up[b]), g["U"][b].astype(np.float64), 1e-8)
    with ThreadPoolExecutor(8) as ex:
        rows = list(ex.map(one, range(B)))
    c = {k: np.array([row[k] for row in rows]) for k in CT.KEYS}
    # the bounds test_certify.py holds the compile-time horizons N = 28 ... 50 to (module docstring there): 1e-7 reference-scaled, 2e-6 on the STRICT scale, which
    # at long horizons is up to ~300x smaller than the one the solve converged on (measured here: 1.2e-6 strict, 4.9e-9 reference-scaled)
    _assert_certified(c, 2e-6, 1e-8 + 1e-12, "wide frenet<double,50>")


@pytest.mark.gpu
@pytest.mark.parametrize("opts", [dict(indef_strategy=0), dict(indef_strategy=1), dict(hessian=0)])
def test_frenet_wide_hessian_strategies(opts):
    N, B = 40, 256
    z0, kp, vt, up = _long_cases(B, N, seed=13)
    ref = _solve(N, z0, kp, vt, up)
    g = _solve(N, z0, kp, vt, up, **opts)
    assert (ref["status"] == 0).all() and (g["status"] == 0).all(), (opts, np.bincount(g["status"]))
    assert (np.abs(g["cost"] - ref["cost"]) / np.maximum(1.0, np.abs(ref["cost"]))).max() <= 1e-7, opts


@pytest.mark.gpu
def test_frenet_wide_warm_start():
    N, B = 50, 256
    z0, kp, vt, up = _long_cases(B, N, seed=29)
    cold = _solve(N, z0, kp, vt, up)
    warm = _solve(N, z0, kp, vt, up, warm_U=cold["U"])
    assert (cold["status"] == 0).all() and (warm["status"] == 0).all()
    # the warm solve starts at the cold solve's answer and may only go further down into the same minimum: never above it (1e-9), and within the
    # warm-start tolerance of test_gpu_parity.py (measured: up to 2e-7 lower -- the cold solve stops at a scaled error of 1e-8, not at the minimum)
    rel = (warm["cost"] - cold["cost"]) / np.maximum(1.0, np.abs(cold["cost"]))
    assert rel.max() <= 1e-9 and rel.min() >= -1e-6, (rel.min(), rel.max())
    # (the shared warm start begins at barrier parameter warm_mu = 1e-6: measured 3 iterations for 51 of 256 problems, 4 for the others, against 8.8 cold)
    assert warm["iters"].max() <= 4 and warm["iters"].mean() < 0.5 * cold["iters"].mean(), np.bincount(warm["iters"])


@pytest.mark.gpu
def test_frenet_wide_module_api(oracle):
    """KinematicMPCFrenet at N = 50: the module-load solve and a few warm-started steps with the reference's argument orders"""
    from mkz_mpc_path_follower_amd.kinematic_mpc_frenet import KinematicMPCFrenet
    O = oracle
    N = 50
    m = KinematicMPCFrenet(N=N)
    assert m.status == "Optimal"
    s_, ey_, v_, epsi_, K_, path_, df_, acc_ = m.get_solver_results()
    assert len(s_) == N + 1 and abs(acc_[0] - 0.15) < 1e-6 and np.abs(df_).max() < 1e-7 and np.abs(ey_).max() < 1e-9
    kpoly = [1e-7, -2e-5, 1e-3, 0.02]
    p = O.params(N, model=1)
    z, u_prev = [1.5, 0.4, -0.05, 6.0], (0.2, 0.01)
    for step in range(3):
        m.update_init_cond(*z)
        m.update_reference({"x": [0.0], "y": [0.0]}, kpoly, 7.0)
        m.update_current_input(u_prev[1], u_prev[0])   # steer first
        m.update_cost(9.0, 10.0, 0.5, 100.0, 1000.0, 0.0, 0.0)
        a, d, st = m.solve_model()
        assert st == "Optimal", step
        r = O.solve_condensed(p, O.problem_frenet(p, z, kpoly, 7.0, u_prev))
        assert abs(m.cost - r["cost"]) <= 1e-6 * max(1.0, r["cost"]) and abs(a - r["U"][0, 0]) < 1e-6 and abs(d - r["U"][0, 1]) < 1e-6, step
        res = m.get_solver_results()
        assert np.allclose(res[0], r["X"][:, 0], atol=2e-5) and np.allclose(res[2], r["X"][:, 3], atol=2e-5)
        z, u_prev = [float(v) for v in r["X"][1]], (a, d)   # advance along the prediction


@pytest.mark.gpu
def test_frenet_wide_containment_and_determinism():
    N, B = 50, 96
    z0, kp, vt, up = _long_cases(B, N, seed=37)
    a = _solve(N, z0, kp, vt, up)
    b = _solve(N, z0, kp, vt, up)
    assert (a["status"] == 0).all()
    for k in ("U", "X", "cost", "viol", "iters", "status", "u0"):
        assert np.array_equal(a[k], b[k]), k
    i = 11
    one = _solve(N, z0[i:i + 1], kp[i:i + 1], vt[i:i + 1], up[i:i + 1])
    for k in ("U", "X", "cost", "viol", "iters", "status", "u0"):
        assert np.array_equal(one[k][0], a[k][i]), k
    kp2 = kp.copy()
    kp2[5, 1] = np.nan
    c = _solve(N, z0, kp2, vt, up)
    assert c["status"][5] != 0
    rest = np.arange(B) != 5
    for k in ("U", "X", "cost", "viol", "iters", "status", "u0"):
        assert np.array_equal(c[k][rest], a[k][rest]), k


@pytest.mark.gpu
def test_slack_guard_trips_in_the_frenet_four_wave_kernel():
    """the run-time slack guard of ipm::solve in the new kernel: with the TEST build libkmpc_hip_corrupt.so no solve may end Optimal (child process)"""
    import json
    import subprocess
    lib = os.path.join(ROOT, "mkz_mpc_path_follower_amd", "libkmpc_hip_corrupt.so")
    assert os.path.exists(lib), "build it: make -C mkz_mpc_path_follower_amd/csrc (the default target builds it)"
    r = subprocess.run([sys.executable, os.path.join(HERE, "_corrupt_probe_frenet.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("CORRUPT_PROBE ")][-1]
    n_opt, n_lim, n_inf, n_err = json.loads(line[len("CORRUPT_PROBE "):])["wide_frenet_f64_N50"]
    assert n_opt == 0 and n_lim == 0 and n_inf == 0 and n_err > 0, (n_opt, n_lim, n_inf, n_err)
