"""GPU tests of the Cholesky block step of the one-wave solve kernel (chol_blocks, Chol4::inv_col), of the retry re-entry of ipm::solve and of the
start-order pre-pass: the KKT pipeline at every tile shape, bit-identity of retried solves against outputs recorded from the parent build, and the
pre-pass leaving every output as it is."""
import os

import numpy as np
import pytest
import torch

from mkz_mpc_path_follower_amd.synthetic import make_batch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "factor_step_parent.npz")
BENCH_SEED = 20180620 + 2
# the pre-pass is two launches at every batch size; 16384 / 16385 stand in for the two sides of a one-launch threshold, should one come
SCHED_SPLIT_B = 16384


def _solver(N, dtype=torch.float64, **kw):
    from mkz_mpc_path_follower_amd import BatchMPC
    return BatchMPC(N=N, dtype=dtype, **kw)


def _kkt_inputs(N, B, f64):
    d = make_batch(B, N, cfg_id=7, seed=4321 + N)
    rng = np.random.default_rng(11 + N)
    U = np.stack([rng.uniform(-0.8, 0.8, (B, N)), rng.uniform(-0.3, 0.3, (B, N))], axis=-1)
    w = 10.0 ** rng.uniform(-2, 6 if f64 else 3, (B, 5 * N - 2))
    bb = rng.normal(0, 1, (B, 2 * N))
    return d, U, w, bb


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("N", [8, 20, 28])
def test_kkt_pipeline_at_every_tile_shape(N, dtype):
    """kmpc_debug_kkt at 2, 3 and 4 tile rows (N = 8, 20, 28: every chol_blocks<TJ> instantiation, 4 / 10 / 14 diagonal blocks), B = 32: the factor and the
    block-LDL^T substitutions solve the matrix the kernel assembled -- x against numpy's solve of the returned K with the returned gradient, to the
    tolerance tests/test_gpu_kernels.py asks of the same quantity (1e-6 in fp64, 2e-2 in fp32, relative to max |x|), and ok == 1 everywhere (Gauss-Newton
    matrix plus a positive shift: positive definite by construction; with the exact Hessian at these random inputs most of the 32 matrices are not).
    Then reg = 0 with the exact Hessian and no barrier weights: every returned K that is indefinite on the CPU (smallest eigenvalue below -1e-9 max |K|,
    -1e-4 in fp32, and numpy's Cholesky refuses it) must come back as ok == 0, and at least one of the 32 is."""
    B, f64 = 32, dtype == torch.float64
    sc, reg = 0.37, 2.5
    d, U, w, bb = _kkt_inputs(N, B, f64)
    s = _solver(N, dtype)
    K, g, x, ok = s.debug_kkt(d["z0"], d["ref"], d["v_target"], d["u_prev"], U, w, bb, sc=sc, reg=reg, hessian=0)
    K, g, x, ok = K.double().cpu().numpy(), g.double().cpu().numpy(), x.double().cpu().numpy(), ok.cpu().numpy()
    assert (ok == 1).all(), ok
    worst = 0.0
    for b in range(B):
        xr = np.linalg.solve(K[b], bb[b] - sc * g[b])
        err = np.abs(x[b] - xr).max() / max(1e-12, np.abs(xr).max())
        worst = max(worst, err)
        assert err <= (1e-6 if f64 else 2e-2), (b, err)
    print("N=%d %s: worst relative error of x %.3e" % (N, "f64" if f64 else "f32", worst))
    # reg = 0 (the interface takes no negative shift), exact Hessian, no barrier weights, inputs far from any minimum
    K2, _, _, ok2 = s.debug_kkt(d["z0"], d["ref"], d["v_target"], d["u_prev"], U, np.zeros_like(w), bb, sc=1.0, reg=0.0, hessian=1)
    K2, ok2 = K2.double().cpu().numpy(), ok2.cpu().numpy()
    n_indef = 0
    for b in range(B):
        ev = np.linalg.eigvalsh(K2[b]).min()
        if ev < -(1e-9 if f64 else 1e-4) * np.abs(K2[b]).max():
            with pytest.raises(np.linalg.LinAlgError):   # indefinite on the CPU too
                np.linalg.cholesky(K2[b])
            n_indef += 1
            assert ok2[b] == 0, (b, ev)
    assert n_indef >= 1, "reg = 0 leaves no indefinite matrix at N = %d: choose other inputs" % N


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _bits(a):
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


@pytest.mark.parametrize("case,N,f32", [("N20_f64", 20, False), ("N20_f32", 20, True), ("N8_f64", 8, False), ("N28_f64", 28, False)])
def test_outputs_bit_identical_to_the_parent_build(golden, case, N, f32):
    """64 problems of bench draw 0 (make_batch(4096, N, cfg_id=2, seed=20180620 + 2); rows 1693, 533, 273, 1330, 3694 and 59 evenly spaced ones) give the
    bit patterns tools/record_factor_step_golden.py recorded from the parent commit's build: u0, cost, iters, status.  The shipped build has no retry
    counter; the recording script counted, with the parent's trace build, the factorisation retries of the five named rows at N = 20 in fp64 and stored
    them in the fixture: 8, 4, 0, 5 and 6 retries (row 1693: 8 over its 18 iterations, up to 2 in one iteration; row 3694: 5 in its second iteration)
    -- so the recorded solves go through the retry re-entry."""
    d = make_batch(4096, N, cfg_id=2, seed=BENCH_SEED, dtype=np.float32 if f32 else np.float64)
    rows = golden["rows"]
    assert len(rows) == 64 and len(set(rows.tolist())) == 64 and rows[0] == 1693
    s = _solver(N, torch.float32 if f32 else torch.float64)
    o = s.solve(d["z0"][rows], d["ref"][rows], d["v_target"][rows], d["u_prev"][rows])
    torch.cuda.synchronize()
    for k in ("u0", "cost", "iters", "status"):
        got, want = o[k].cpu().numpy(), golden[case + "_" + k]
        assert got.dtype == want.dtype and got.shape == want.shape, k
        diff = np.flatnonzero((_bits(got) != _bits(want)).reshape(len(rows), -1).any(axis=1))
        assert diff.size == 0, "%s of rows %s differs from the parent build" % (k, rows[diff].tolist())
    retries = golden["retries_named_N20_f64"]
    assert retries.shape == (5,) and retries[0] >= 1 and retries.sum() == 23, retries


def _solve_np(s, d):
    o = s.solve(d["z0"], d["ref"], d["v_target"], d["u_prev"], want_U=True)
    torch.cuda.synchronize()
    return {k: o[k].cpu().numpy() for k in ("u0", "U", "cost", "viol", "iters", "status")}


def _same(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)


def test_start_order_prepass_does_not_change_results():
    """The start order changes when a problem starts, never what it computes: with `schedule` on and off the same batch gives bitwise equal outputs at
    B = 2049 (the first batch that takes the pre-pass), 4096, 16384 and 16385 -- a wrong or incomplete permutation solves some problem twice and
    another not at all.  N = 8 keeps the large batches short.  Then one handle in sequence: the same batch twice (histogram parity), other batch sizes,
    and the first size again."""
    N, T = 8, SCHED_SPLIT_B
    d = make_batch(T + 1, N, cfg_id=2, seed=77)
    cut = lambda B: {k: d[k][:B] for k in ("z0", "ref", "v_target", "u_prev")}
    on, off = _solver(N, schedule=1), _solver(N, schedule=0)
    ref = {}
    for B in (2049, 4096, T, T + 1):
        ref[B] = _solve_np(off, cut(B))
        assert _same(_solve_np(on, cut(B)), ref[B]), B
    seq = _solver(N, schedule=1)
    for B in (4096, 4096, T + 1, T + 1, 4096, T, 2049):
        assert _same(_solve_np(seq, cut(B)), ref[B]), B
