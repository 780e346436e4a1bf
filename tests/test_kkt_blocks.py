"""GPU block tests of the KKT pipeline on the paths tests/test_gpu_kernels.py and tests/test_factor_step.py do not reach: the shared Frenet functor
(ipm::eval_frenet / linearize_frenet) with its three condensings -- the MFMA contraction of the one-wave kernel, the classical P_k recursion of the
four-wave kernel and of the four-per-wave kernel -- the whole KKT back-end of the four-per-wave kernel for both models (one matrix row per lane, the
16-step Cholesky, the 4x4 block inverses, fwd_block / back_block), and the generic kernel's own Frenet functor.

Everything is compared with the CPU oracle: K against sc * H_oracle + A^T diag(w) A + reg * I, the gradient against the oracle's, x against numpy's
solve of that system -- the assertions and the bounds of test_kkt_pipeline_of_the_solve_kernels.  An end-to-end solve cannot see an error in K: an
interior-point method with the right gradient and a wrong Hessian ends at the same point a few iterations later.

fp32 cases evaluate the oracle at the inputs rounded to fp32 and back: the kernel is not charged for the rounding of its inputs.

The inputs must meet conditions of their own, asserted here on the CPU reference alone (seeds and ranges were chosen so that it does):
  * 1 - e_y K(s) >= 0.2 at every stage of the oracle's roll-out (the Frenet frame is singular at 0);
  * with the Gauss-Newton matrix every K_ref is positive definite, with the exact Hessian at least half of them are;
  * the reg = 0, w = 0, exact-Hessian pass has at least one matrix that is indefinite on the CPU;
  * four-per-wave cases: at least one wave holds an indefinite and a positive definite problem side by side, in the main pass and in the reg = 0 pass.
"""
import functools

import numpy as np
import pytest
import torch

from mkz_mpc_path_follower_amd.synthetic import make_batch
from test_frenet import _cases
from test_gpu_kernels import _forms_matrix

pytestmark = pytest.mark.gpu

SC, REG = 0.37, 2.5
SEED = 21
QUAD_CARTESIAN_B = 1027   # the first batch sizes that select the four-per-wave kernel start at 1024; 1027 leaves the last wave one live row
# path -> (model, handle options, B)
PATHS = {"fast_frenet": (1, {}, 6), "wide_frenet": (1, {}, 6), "quad_frenet": (1, {"kernel_variant": 3}, 30), "quad_cartesian": (0, {}, QUAD_CARTESIAN_B)}
# lower end of the exponent of w where -2, the value of test_kkt_pipeline_of_the_solve_kernels, leaves fewer than half of the exact-Hessian matrices
# positive definite on the CPU (2 of 6, 2 of 6, 0 of 6): the smallest integer that gives half
W_LO = {("fast_frenet", 28, False): -1, ("wide_frenet", 32, True): -1, ("wide_frenet", 50, True): 4}
CASES = ([("fast_frenet", N, True) for N in (8, 12, 16, 20, 24, 28)] + [("fast_frenet", N, False) for N in (8, 20, 28)] +
         [("wide_frenet", N, True) for N in (32, 40, 50)] +
         [("quad_frenet", 8, True), ("quad_frenet", 8, False), ("quad_cartesian", 8, True), ("quad_cartesian", 8, False)])


def _r32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _inputs(path, N, f64, seed=SEED):
    """the drawn problem data and evaluation point, as the kernel sees them (fp32 cases: rounded to fp32 and back)"""
    model, _, B = PATHS[path]
    if model == 1:
        z0, second, vt, up = _cases(B, N, seed=seed)
    else:
        d = make_batch(B, N, cfg_id=7, seed=4321 + seed)
        z0, second, vt, up = d["z0"], d["ref"], d["v_target"], d["u_prev"]
    rng = np.random.default_rng(11 + N + 1000 * (seed - SEED))
    U = np.stack([rng.uniform(-0.8, 0.8, (B, N)), rng.uniform(-0.3, 0.3, (B, N))], axis=-1)
    w = 10.0 ** rng.uniform(W_LO.get((path, N, f64), -2), 6 if f64 else 3, (B, 5 * N - 2))
    bb = rng.normal(0, 1, (B, 2 * N))
    a = dict(z0=z0, second=second, vt=vt, up=up, U=U, w=w, bb=bb)
    if not f64:
        a = {k: _r32(v) for k, v in a.items()}
    return a


def _oracle_blocks(O, path, N, a):
    """per problem: Gauss-Newton and exact condensed Hessian, gradient, and the smallest 1 - e_y K(s) of the roll-out (Frenet)"""
    model, _, B = PATHS[path]
    p = O.params(N, model=model)
    H0, H1, g, den = [], [], [], []
    for b in range(B):
        if model == 1:
            q = O.problem_frenet(p, a["z0"][b], a["second"][b], a["vt"][b], a["up"][b])
            X = O.rollout(p, a["z0"][b], a["U"][b], a["second"][b])
            den.append((1.0 - X[:, 1] * np.polyval(a["second"][b], X[:, 0])).min())
        else:
            q = O.problem(p, a["z0"][b], a["second"][b], a["vt"][b], a["up"][b])
            den.append(1.0)
        h0, _, _ = O.condense(p, q, a["U"][b], hessian=0)
        h1, gg, _ = O.condense(p, q, a["U"][b], hessian=1)
        H0.append(h0); H1.append(h1); g.append(gg)
    return dict(H=(np.array(H0), np.array(H1)), g=np.array(g), den=np.array(den), dt=p.dt)


@functools.lru_cache(maxsize=None)
def _reference(path, N, f64):
    """inputs and oracle blocks of one case, computed once and shared by its two `hessian` parametrisations; nobody writes to them"""
    from oracle import oracle as O
    a = _inputs(path, N, f64)
    r = _oracle_blocks(O, path, N, a)
    A = _forms_matrix(N, dt=r["dt"])
    r["G"] = np.einsum("fi,bf,fj->bij", A, a["w"], A)   # A^T diag(w) A
    for v in (r["G"], r["g"], r["den"], r["H"][0], r["H"][1]):
        v.setflags(write=False)
    return a, r


def _kref(r, hessian, sc, reg, with_forms=True):
    n = r["g"].shape[1]
    return sc * r["H"][hessian] + (r["G"] if with_forms else 0.0) + reg * np.eye(n)


def _indefinite(K, f64):
    return np.linalg.eigvalsh(K).min() < -(1e-9 if f64 else 1e-4) * np.abs(K).max()


def _mixed_wave(indef, pd):
    """a wave of the four-per-wave kernel (four consecutive problems) that holds an indefinite and a positive definite problem"""
    B = len(indef)
    return any(indef[i:i + 4].any() and pd[i:i + 4].any() for i in range(0, B, 4))


def _solver(path, N, f64):
    from mkz_mpc_path_follower_amd import BatchMPC
    model, kw, _ = PATHS[path]
    return BatchMPC(N=N, dtype=torch.float64 if f64 else torch.float32, model=model, **kw)


def _run(s, a, w, sc, reg, hessian):
    out = s.debug_kkt(a["z0"], a["second"], a["vt"], a["up"], a["U"], w, a["bb"], sc=sc, reg=reg, hessian=hessian)
    torch.cuda.synchronize()
    K, g, x, ok = out
    return K.double().cpu().numpy(), g.double().cpu().numpy(), x.double().cpu().numpy(), ok.cpu().numpy()


@pytest.mark.parametrize("path,N,f64", CASES, ids=["%s-N%d-%s" % (p, N, "f64" if f else "f32") for p, N, f in CASES])
@pytest.mark.parametrize("hessian", [0, 1])
def test_kkt_blocks_match_oracle(path, N, f64, hessian):
    """kmpc_debug_kkt on the Frenet functor in the one-wave kernel (every compiled horizon), in the four-wave kernel (5, 6 and 7 tile rows) and in the
    four-per-wave kernel (B = 30: eight waves, the last with two spare rows), and on the Cartesian four-per-wave kernel at the first batch size that
    selects it and is no multiple of four (B = 1027, every row checked).  Bounds of test_kkt_pipeline_of_the_solve_kernels, unchanged:
    fp64 |K - K_ref| <= 1e-10 max|K_ref|, gradient 1e-9, residual of x 1e-9, x against numpy's solve 1e-6; fp32 2e-5 / 1e-4 / 2e-3 sqrt(cond) / 2e-2.
    Where K_ref is positive definite ok == 1; an indefinite K_ref comes back ok == 0 (bar: smallest eigenvalue below -1e-9 max|K| in fp64, -1e-4 in
    fp32, and numpy's Cholesky refuses it).  Exact Hessian: a second pass with reg = 0, w = 0, sc = 1 -- K, gradient and the flag; in the four-per-wave
    kernel the positive definite problems that share a wave with an indefinite one are held to the same bounds as every other (rows of a wave do not
    disturb each other).  The worst observed value of each quantity is printed."""
    a, r = _reference(path, N, f64)
    B, n = a["U"].shape[0], 2 * N
    quad = path.startswith("quad")
    tK, tg, tr, tx = (1e-10, 1e-9, 1e-9, 1e-6) if f64 else (2e-5, 1e-4, 2e-3, 2e-2)
    # ---- conditions on the inputs, on the CPU reference alone
    assert r["den"].min() >= 0.2, "1 - e_y K(s) gets as low as %.3f: narrow the drawn inputs" % r["den"].min()
    Kr = _kref(r, hessian, SC, REG)
    ev = np.array([np.linalg.eigvalsh(k).min() for k in Kr])
    pd = ev > 0
    indef = np.array([_indefinite(k, f64) for k in Kr])
    if hessian == 0:
        assert pd.all(), "Gauss-Newton matrix plus a shift must be positive definite"
    else:
        assert 2 * pd.sum() >= B, "only %d of %d matrices are positive definite: raise the lower end of w" % (pd.sum(), B)
        if quad:
            assert _mixed_wave(indef, pd), "no wave holds an indefinite and a definite problem: choose other inputs"
    # ---- the kernel
    s = _solver(path, N, f64)
    K, g, x, ok = _run(s, a, a["w"], SC, REG, hessian)
    worst = dict(K=0.0, g=0.0, res=0.0, x=0.0)
    for b in range(B):
        go = r["g"][b]
        eK = np.abs(K[b] - Kr[b]).max() / np.abs(Kr[b]).max()
        eg = np.abs(g[b] - go).max() / max(1.0, np.abs(go).max())
        worst["K"], worst["g"] = max(worst["K"], eK), max(worst["g"], eg)
        assert eK <= tK, (b, eK)
        assert eg <= tg, (b, eg)
        if pd[b]:
            assert ok[b] == 1, (b, ev[b])
            rhs = a["bb"][b] - SC * go
            eres = np.abs(Kr[b] @ x[b] - rhs).max() / (max(1.0, np.abs(rhs).max()) * (1.0 if f64 else np.sqrt(np.linalg.cond(Kr[b]))))
            xr = np.linalg.solve(Kr[b], rhs)
            ex = np.abs(x[b] - xr).max() / max(1e-12, np.abs(xr).max())
            worst["res"], worst["x"] = max(worst["res"], eres), max(worst["x"], ex)
            assert eres <= tr, (b, eres)
            assert ex <= tx, (b, ex)
        elif indef[b]:
            with pytest.raises(np.linalg.LinAlgError):
                np.linalg.cholesky(Kr[b])
            assert ok[b] == 0, (b, ev[b])
    print("%s N=%d %s hessian=%d: worst K %.2e  g %.2e  residual %.2e  x %.2e  (%d of %d positive definite)"
          % (path, N, "f64" if f64 else "f32", hessian, worst["K"], worst["g"], worst["res"], worst["x"], pd.sum(), B))
    if hessian == 0:
        return
    # ---- reg = 0 (the interface takes no negative shift), exact Hessian, no barrier weights, inputs far from any minimum
    K0r = _kref(r, 1, 1.0, 0.0, with_forms=False)
    indef0 = np.array([_indefinite(k, f64) for k in K0r])
    pd0 = np.array([np.linalg.eigvalsh(k).min() > (1e-9 if f64 else 1e-4) * np.abs(k).max() for k in K0r])
    assert indef0.any(), "reg = 0 leaves no indefinite matrix: choose other inputs"
    if quad:
        assert _mixed_wave(indef0, pd0), "reg = 0: no wave holds an indefinite and a definite problem: choose other inputs"
    K0, g0, _, ok0 = _run(s, a, np.zeros_like(a["w"]), 1.0, 0.0, 1)
    wK = 0.0
    for b in range(B):
        eK = np.abs(K0[b] - K0r[b]).max() / np.abs(K0r[b]).max()
        wK = max(wK, eK)
        assert eK <= tK, (b, eK)
        assert np.abs(g0[b] - r["g"][b]).max() <= tg * max(1.0, np.abs(r["g"][b]).max()), b
        if indef0[b]:
            with pytest.raises(np.linalg.LinAlgError):
                np.linalg.cholesky(K0r[b])
            assert ok0[b] == 0, b
        elif pd0[b]:
            assert ok0[b] == 1, b
    print("%s N=%d %s reg=0: worst K %.2e  (%d of %d indefinite, %d positive definite)"
          % (path, N, "f64" if f64 else "f32", wK, indef0.sum(), B, pd0.sum()))


@pytest.mark.parametrize("N", [8, 13, 24])
@pytest.mark.parametrize("hessian", [0, 1])
def test_generic_frenet_condense_matches_oracle(oracle, N, hessian):
    """The generic kernel's own Frenet functor -- Solver<T,NT,1>::eval_frenet, linearize_frenet, condense_dense, a second implementation of the same
    derivatives -- at one, two and three column tiles (N = 13: n = 26 fills neither its last tile nor a multiple of four): kmpc_debug_condense on a
    model = 1, kernel_variant = 1 handle against O.condense, with the bounds of test_condense_matches_oracle."""
    from mkz_mpc_path_follower_amd import BatchMPC
    O = oracle
    B = 6
    z0, kp, vt, up = _cases(B, N, seed=SEED)
    rng = np.random.default_rng(5)
    U = np.stack([rng.uniform(-0.8, 0.8, (B, N)), rng.uniform(-0.3, 0.3, (B, N))], axis=-1)
    s = BatchMPC(N=N, dtype=torch.float64, model=1, kernel_variant=1)
    H, g, J = [t.cpu().numpy() for t in s.debug_condense(z0, kp, vt, U, hessian=hessian)]
    p = O.params(N, model=1)
    worst = [0.0, 0.0, 0.0]
    for b in range(B):
        q = O.problem_frenet(p, z0[b], kp[b], vt[b], up[b])
        Ho, go, Jo = O.condense(p, q, U[b], hessian=hessian)
        e = (abs(J[b] - Jo) / max(1.0, abs(Jo)), np.abs(g[b] - go).max() / max(1.0, np.abs(go).max()), np.abs(H[b] - Ho).max() / np.abs(Ho).max())
        worst = [max(u, v) for u, v in zip(worst, e)]
        assert e[0] <= 1e-10 and e[1] <= 1e-9 and e[2] <= 1e-10, (b, e)
    print("generic_frenet_condense N=%d hessian=%d: worst J %.2e  g %.2e  H %.2e" % (N, hessian, *worst))


def test_refusals_of_the_diagnostics():
    """The four-wave Frenet kernel is fp64 only: a model = 1 handle at a four-wave horizon in fp32 is refused when it is created, so kmpc_debug_kkt
    never meets one; kmpc_debug_condense refuses a Frenet handle whose horizon the generic kernel's Frenet functor is not built for."""
    from mkz_mpc_path_follower_amd import BatchMPC, _lib
    with pytest.raises(_lib.KmpcError, match="fp64 only"):
        BatchMPC(N=32, dtype=torch.float32, model=1)
    N, B = 28, 2
    z0, kp, vt, up = _cases(B, N, seed=SEED)
    s = BatchMPC(N=N, dtype=torch.float64, model=1)
    with pytest.raises(_lib.KmpcError, match="N <= 24"):
        s.debug_condense(z0, kp, vt, np.zeros((B, N, 2)), hessian=0)
