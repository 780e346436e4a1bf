"""CPU tests of the oracle (oracle/): known answers, quirks of the reference NLP, derivative checks,
agreement with the committed golden fixtures.  The reference has no tests of its own."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(__file__), "golden")
NODE_W = (9.0, 9.0, 10.0, 0.0, 100.0, 1000.0, 0.0, 0.0)


def line_ref(N, v=15.0, dt=0.2):
    r = np.zeros((N + 1, 3))
    r[:, 0] = v * dt * np.arange(N + 1)
    return r


@pytest.mark.parametrize("N", [8, 20, 50])
def test_on_path_at_speed_is_zero(oracle, N):
    O = oracle
    p = O.params(N)
    r = O.solve_condensed(p, O.problem(p, [0, 0, 0, 15.0], line_ref(N), 15.0))
    assert r["status"] == 0 and abs(r["cost"]) < 1e-12 and np.abs(r["U"]).max() < 1e-7


@pytest.mark.parametrize("N,J", [(8, 15738.467), (20, 194745.62), (50, 2050558.8)])
def test_module_load_problem(oracle, N, J):
    """BASELINE config 1 (MKZMPCPathFollower.jl:36-39,110-113,127): standing start, straight reference.
    Pure QP in acc; first-step rate bound a_dmax*dt_control = 0.15 is active (Q2)."""
    O = oracle
    p = O.params(N)
    r = O.solve_condensed(p, O.problem(p, [0, 0, 0, 0.0], line_ref(N), 15.0))
    assert r["status"] == 0
    assert abs(r["cost"] - J) < 1e-7 * J
    assert abs(r["U"][0, 0] - 0.15) < 2e-8 and np.abs(r["U"][:, 1]).max() < 1e-9
    # Q1: the pair u_2 - u_1 is NOT rate constrained -> the optimum jumps by more than a_dmax*dt = 0.3
    assert r["U"][1, 0] - r["U"][0, 0] > 0.3 + 1e-3
    # later pairs are constrained
    assert np.all(np.abs(np.diff(r["U"][1:, 0])) <= 0.3 + 1e-7)


def test_first_step_bounds_active(oracle):
    O = oracle
    p = O.params(8)
    r = O.solve_condensed(p, O.problem(p, [0, 1.0, 0.1, 10.0], line_ref(8), 15.0))
    assert abs(r["U"][0, 0] - 0.15) < 2e-8 and abs(r["U"][0, 1] + 0.05) < 2e-8
    assert abs(r["cost"] - 1692.89097) < 1e-4


def test_mirror_and_rigid_motion_invariance(oracle):
    """mirroring y/psi flips d_f; rotation + translation leave U*, J* unchanged (C_x = C_y)."""
    O = oracle
    N = 8
    p = O.params(N, NODE_W)
    ref = line_ref(N, 10.0)
    z0 = np.array([0.0, 0.8, 0.05, 9.0])
    r0 = O.solve_condensed(p, O.problem(p, z0, ref, 10.0, (0.1, 0.02)))
    m = np.array([1.0, -1.0, -1.0])
    r1 = O.solve_condensed(p, O.problem(p, z0 * np.array([1, -1, -1, 1]), ref * m, 10.0, (0.1, -0.02)))
    assert abs(r0["cost"] - r1["cost"]) < 1e-7 * r0["cost"]
    assert np.abs(r0["U"][:, 0] - r1["U"][:, 0]).max() < 1e-5 and np.abs(r0["U"][:, 1] + r1["U"][:, 1]).max() < 1e-5
    th, t = 0.7, np.array([3.0, -2.0])
    Rm = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    ref2 = ref.copy()
    ref2[:, :2] = ref[:, :2] @ Rm.T + t
    ref2[:, 2] += th
    z2 = z0.copy()
    z2[:2] = Rm @ z0[:2] + t
    z2[2] += th
    r2 = O.solve_condensed(p, O.problem(p, z2, ref2, 10.0, (0.1, 0.02)))
    assert abs(r0["cost"] - r2["cost"]) < 1e-7 * r0["cost"]
    assert np.abs(r0["U"] - r2["U"]).max() < 1e-5


def test_quirks_dead_inputs(oracle):
    """Q3: x_r[1], y_r[1], psi_r[1] are dead inputs; terminal v is not in the C_v term."""
    O = oracle
    N = 8
    w = list(NODE_W)
    w[3] = 5.0  # C_v > 0 so the speed term matters
    p = O.params(N, w)
    ref = line_ref(N, 10.0)
    q = O.problem(p, [0, 0.2, 0, 8.0], ref, 10.0)
    r0 = O.solve_condensed(p, q)
    ref2 = ref.copy()
    ref2[0] = [123.0, -45.0, 2.0]
    r1 = O.solve_condensed(p, O.problem(p, [0, 0.2, 0, 8.0], ref2, 10.0))
    assert abs(r0["cost"] - r1["cost"]) < 1e-9 * max(1, r0["cost"]) and np.abs(r0["U"] - r1["U"]).max() < 1e-9
    # cost() restated by hand, with the reference's index ranges (:97-103)
    U, X = r0["U"], r0["X"]
    J = sum(w[0] * (X[k, 0] - ref[k, 0]) ** 2 + w[1] * (X[k, 1] - ref[k, 1]) ** 2 + w[2] * (X[k, 2] - ref[k, 2]) ** 2
            for k in range(1, N + 1))
    J += w[3] * sum((X[k, 3] - 10.0) ** 2 for k in range(1, N))  # i = 2:N  -> terminal v excluded
    J += w[4] * np.sum(np.diff(U[:, 0]) ** 2) + w[5] * np.sum(np.diff(U[:, 1]) ** 2)
    assert abs(J - r0["cost"]) < 1e-9 * max(1.0, J)


def test_infeasible_initial_speed(oracle):
    """Q5: v[1] is pinned to v0 and bounded to [0, 20] -> v0 outside is infeasible; output stays finite and in the box."""
    O = oracle
    p = O.params(8)
    r = O.solve_condensed(p, O.problem(p, [0, 0, 0, 25.0], line_ref(8), 15.0))
    assert r["status"] == 2 and np.isfinite(r["U"]).all() and np.abs(r["U"][:, 0]).max() <= 1.0
    r = O.solve_condensed(p, O.problem(p, [0, 0, 0, 0.0], line_ref(8), 15.0, (-0.9, 0.0)))  # standing, hard braking held
    assert r["status"] == 2


@pytest.mark.parametrize("N", [8, 20])
def test_gradient_and_hessian_against_finite_differences(oracle, N):
    O = oracle
    p = O.params(N, (9, 9, 10, 2.0, 100, 1000, 0.5, 3.0))
    rng = np.random.default_rng(3)
    k = np.arange(N + 1)
    ref = np.stack([8 * 0.2 * k, 0.05 * k ** 1.5, 0.02 * k], axis=1)
    q = O.problem(p, [0.1, -0.4, 0.05, 7.0], ref, 8.0)
    U = np.stack([rng.uniform(-0.5, 0.5, N), rng.uniform(-0.2, 0.2, N)], axis=1)
    g = O.grad(p, q, U)
    H, g2, J = O.condense(p, q, U, hessian=1)
    assert np.abs(g - g2).max() < 1e-9 * max(1, np.abs(g).max())
    assert abs(J - O.cost(p, q, U)) < 1e-12 * max(1, J)
    h = 1e-6
    gfd = np.zeros(2 * N)
    Hfd = np.zeros((2 * N, 2 * N))
    for j in range(2 * N):
        e = np.zeros(2 * N)
        e[j] = h
        Up, Um = (U.ravel() + e).reshape(N, 2), (U.ravel() - e).reshape(N, 2)
        gfd[j] = (O.cost(p, q, Up) - O.cost(p, q, Um)) / (2 * h)
        Hfd[:, j] = (O.grad(p, q, Up) - O.grad(p, q, Um)) / (2 * h)
    assert np.abs(g - gfd).max() < 1e-5 * max(1, np.abs(g).max())
    assert np.abs(H - Hfd).max() < 1e-6 * np.abs(H).max()
    assert np.abs(H - H.T).max() < 1e-9 * np.abs(H).max()
    Hgn = O.condense(p, q, U, hessian=0)[0]
    assert np.linalg.eigvalsh(Hgn).min() > -1e-8 * np.abs(Hgn).max()  # Gauss-Newton part is PSD


@pytest.mark.parametrize("N", [8, 20, 50])
def test_condensed_oracle_matches_golden(oracle, N):
    """fixtures: tests/golden/kmpc_N*.npz (oracle/make_golden.py; three solvers agreed to < 2e-7 relative)."""
    O = oracle
    G = np.load(os.path.join(GOLD, "kmpc_N%d.npz" % N))
    p = O.params(N, G["weights"])
    r = O.solve_condensed_batch(p, G["z0"], G["ref"], G["v_target"], G["u_prev"], nthreads=8)
    assert (r["status"] == 0).all()
    Jg = G["J_ipopt_like"]
    assert (np.abs(r["cost"] - Jg) <= 1e-6 * np.maximum(1.0, np.abs(Jg))).all()
    assert np.abs(G["J_scipy"] - Jg).max() <= 2e-7 * np.maximum(1.0, np.abs(Jg)).max()
    assert r["viol"].max() <= 1e-8 + 1e-12
    assert np.abs(r["U"][:, 0, :] - G["U_ipopt_like"][:, 0, :]).max() < 1e-4
    # every solution is a certified KKT point of the state-eliminated NLP
    for b in range(0, len(Jg), 5):
        q = O.problem(p, G["z0"][b], G["ref"][b], G["v_target"][b], G["u_prev"][b])
        rs = O.solve_condensed(p, q)
        c = O.certify(p, q, rs["U"], rs["lam"])
        scale = max(1.0, np.abs(O.grad(p, q, rs["U"])).max())
        assert c["stationarity"] <= 1e-6 * scale and c["violation"] <= 1e-8 + 1e-12 and c["lam_min"] >= 0


@pytest.mark.parametrize("N", [8, 20])
def test_reference_start_option_of_the_checker(oracle, N):
    """opts.start = 1: every input starts at 0 as in the reference (MKZMPCPathFollower.jl:65-72), inside the bounds.  With u_prev = 0 and a
    speed well inside its bounds the start IS the zero vector's neighbourhood: the solve ends in the fixtures' minima at N = 8 / 20."""
    O = oracle
    G = np.load(os.path.join(GOLD, "kmpc_N%d.npz" % N))
    p = O.params(N, G["weights"])
    r = O.solve_condensed_batch(p, G["z0"], G["ref"], G["v_target"], G["u_prev"], o=O.opts(start=1), nthreads=8)
    assert (r["status"] == 0).all()
    Jg = G["J_ipopt_like"]
    assert (np.abs(r["cost"] - Jg) <= 1e-6 * np.maximum(1.0, np.abs(Jg))).all()
    # one iteration from the start: the step direction only -- U after max_iter = 1 differs from 0 by one damped Newton step, and with
    # u_prev = 0, v0 = 5 on a straight reference at 5 m/s the all-zero start is already optimal (J = 0): it must be returned unchanged
    ref = np.zeros((N + 1, 3)); ref[:, 0] = 5.0 * 0.2 * np.arange(N + 1)
    q = O.problem(p, [0.0, 0.0, 0.0, 5.0], ref, 5.0, (0.0, 0.0))
    r1 = O.solve_condensed(p, q, O.opts(start=1))
    assert r1["status"] == 0 and np.abs(r1["U"]).max() < 1e-6 and r1["cost"] < 1e-9


def test_ipopt_like_full_space_matches_golden(oracle):
    """the independent full-space Ipopt-style restatement reproduces the fixtures (N = 8 subset; seconds)."""
    from oracle import ipopt_like as IL
    G = np.load(os.path.join(GOLD, "kmpc_N8.npz"))
    for b in (0, 1, 2, 3, 5, 9, 17):
        r = IL.solve_problem(8, G["z0"][b], G["ref"][b], G["v_target"][b], G["u_prev"][b], weights=tuple(G["weights"]))
        assert r["status"] == 0
        assert abs(r["cost"] - G["J_ipopt_like"][b]) <= 1e-8 * max(1.0, abs(G["J_ipopt_like"][b]))
        assert r["constr_viol"] < 1e-9


def test_warm_start_reaches_same_optimum(oracle):
    O = oracle
    N = 20
    p = O.params(N)
    k = np.arange(N + 1)
    s = 9.0 * 0.2 * k
    ref = np.stack([30 * np.sin(s / 30), 30 * (1 - np.cos(s / 30)), s / 30], axis=1)
    q = O.problem(p, [0, 0.4, 0.02, 8.5], ref, 9.0, (0.1, 0.05))
    cold = O.solve_condensed(p, q)
    warm = O.solve_condensed(p, q, O.opts(warm=1), U0=cold["U"])
    assert warm["status"] == 0 and abs(warm["cost"] - cold["cost"]) < 1e-6 * max(1, cold["cost"])
    assert warm["iters"] <= cold["iters"]


def test_line_search_accepts_steps_below_the_merit_noise(oracle):
    """Round 3: near a low-cost optimum the predicted decrease of phi_mu falls below the noise of its evaluation (~60 eps |phi|) and the Armijo
    test used to fail on rounding alone -- this problem (cost 2.17, error 3.5e-8 after five iterations) then took 8 iterations with 96 trial
    roll-outs, the same problem on the GPU 13-18 iterations and set the time of its 4096-problem launch.  With the noise-aware acceptance
    (KMPC_NOISE_ACCEPT, same rule in csrc/kmpc_ipm.h) it is done in 6 iterations with one trial each."""
    from mkz_mpc_path_follower_amd.synthetic import make_batch
    O = oracle
    d = make_batch(4096, 20, cfg_id=2, seed=20228134)
    b = 1342
    r = O.solve_condensed_batch(O.params(20), d["z0"][b:b + 1], d["ref"][b:b + 1], d["v_target"][b:b + 1], d["u_prev"][b:b + 1], nthreads=1)
    assert r["status"][0] == 0 and abs(r["cost"][0] - 2.169311511528) < 1e-9
    assert r["iters"][0] <= 7 and r["n_ls"][0] <= 8, (r["iters"], r["n_ls"])


def test_barrier_floor_gate_keeps_the_cycling_problem(oracle):
    """Round 3: the Mehrotra target's floor mu >= rd / 1000 is dropped (outside shift mode) while the optimality error fell in each of the last two
    iterations.  Without any floor there this problem of the N = 50 bench batch cycles to the iteration cap (mu collapses to 1e-8 at error 5, a 3 % step,
    the error rebounds); its error never falls twice in a row, so the gate keeps its floor: Optimal in 15 iterations, cost 802.09 (the cycle sat at 814)."""
    from mkz_mpc_path_follower_amd.synthetic import make_batch
    O = oracle
    d = make_batch(4096, 50, cfg_id=5)
    b = 1010
    r = O.solve_condensed_batch(O.params(50), d["z0"][b:b + 1], d["ref"][b:b + 1], d["v_target"][b:b + 1], d["u_prev"][b:b + 1], nthreads=1)
    assert r["status"][0] == 0 and r["iters"][0] <= 20 and abs(r["cost"][0] - 802.0932995) < 1e-5, (r["status"], r["iters"], r["cost"])


def test_degenerate_pair_rule_shortens_the_end_game(oracle):
    """Round 3: a standing start whose optimum accelerates at the limit to the end of the horizon -- the bound of the last acceleration input is active with a zero
    multiplier (only the rate cost ties a_{N-1} to a_{N-2}), slack and multiplier vanish together and Newton's method shrinks them x0.375 per iteration.  With the
    pair's barrier stiffness scaled by theta = 0.6 once it is seen shrinking that way: 16 iterations instead of 19, same cost."""
    from mkz_mpc_path_follower_amd.synthetic import make_batch
    O = oracle
    d = make_batch(4096, 20, cfg_id=2)
    b = 3694
    args = (O.params(20), d["z0"][b:b + 1], d["ref"][b:b + 1], d["v_target"][b:b + 1], d["u_prev"][b:b + 1])
    r = O.solve_condensed_batch(*args, nthreads=1)
    r0 = O.solve_condensed_batch(*args, o=O.opts(degen_theta=1.0), nthreads=1)
    assert r["status"][0] == 0 and r0["status"][0] == 0 and r["iters"][0] <= r0["iters"][0] - 2, (r["iters"], r0["iters"])
    assert abs(r["cost"][0] - r0["cost"][0]) <= 1e-8 * abs(r0["cost"][0])
    assert np.abs(r["U"][0, 1:, 0] - 1.0).max() <= 1e-4  # the whole horizon at a_max (but the rate-limited first step)


def test_wrong_point_warm_start_with_a_tiny_barrier_does_not_crawl(oracle):
    """Round 3: warm start from the solution of an unrelated problem with warm_mu = 1e-7 (not the default 1e-6): slacks 1e-5 off the bounds, mu_cur ~ 3e-5 and a
    dual infeasibility of 100 -- every step is a 1e-6 fraction-to-the-boundary step and mu, capped at mu_cur, can never grow: 200 iterations without the rule
    that lifts the cap after a tiny step."""
    from mkz_mpc_path_follower_amd.synthetic import make_batch
    O = oracle
    N, B, i = 8, 32768, 2310
    a, b = make_batch(B, N, cfg_id=5), make_batch(B, N, cfg_id=6)
    p = O.params(N)
    ra = O.solve_condensed_batch(p, a["z0"][i:i + 1], a["ref"][i:i + 1], a["v_target"][i:i + 1], a["u_prev"][i:i + 1], nthreads=1)
    o = O.opts()
    o.warm, o.warm_mu, o.warm_push = 1, 1e-7, 1e-5
    args = (p, b["z0"][i:i + 1], b["ref"][i:i + 1], b["v_target"][i:i + 1], b["u_prev"][i:i + 1])
    rw = O.solve_condensed_batch(*args, o=o, U0=ra["U"].reshape(1, -1), nthreads=1)
    rc = O.solve_condensed_batch(*args, nthreads=1)
    assert rw["status"][0] == 0 and rw["iters"][0] <= 25 and abs(rw["cost"][0] - rc["cost"][0]) <= 1e-6 * max(1.0, abs(rc["cost"][0])), (rw["status"], rw["iters"])
    o.unstick = 0.0
    r0 = O.solve_condensed_batch(*args, o=o, U0=ra["U"].reshape(1, -1), nthreads=1)
    assert r0["status"][0] == 1 and r0["iters"][0] == o.max_iter, (r0["status"], r0["iters"])


@pytest.mark.parametrize("N,count", [(8, 36), (20, 33), (50, 33)])
def test_scenario_fixture_is_what_the_oracle_computes(oracle, N, count):
    """tests/golden/kmpc_scenario_N{8,20,50}.npz (oracle/make_scenario_fixture.py [N]): 36 / 33 / 33 MPC problems met by the closed loop on the reference's own launch scenario
    (standing start, transient, steady tracking, the Q8 garbage-heading periods, the bunched waypoints at the path's end) at the reference's horizon and at those of BASELINE
    configs[1] and configs[4], each solved cold by the full-space Ipopt restatement, the condensed port and scipy (agreement 2e-7): the port reproduces its stored answers and
    the three stored costs agree"""
    O = oracle
    G = np.load(os.path.join(GOLD, "kmpc_scenario_N%d.npz" % N))
    assert int(G["N"]) == N and len(G["J_ipopt_like"]) >= count and any("step_439" in n for n in G["names"]) and any("step_0" == n[-6:] for n in G["names"])
    p = O.params(N, G["weights"])
    r = O.solve_condensed_batch(p, G["z0"], G["ref"], G["v_target"], G["u_prev"], nthreads=4)
    assert (r["status"] == 0).all()
    scale = np.maximum(1.0, np.abs(G["J_ipopt_like"]))
    assert (np.abs(r["cost"] - G["J_condensed"]) / scale).max() <= 1e-9
    assert (np.abs(G["J_condensed"] - G["J_ipopt_like"]) / scale).max() < 2e-7 and (np.abs(G["J_scipy"] - G["J_ipopt_like"]) / scale).max() < 2e-7
    assert np.abs(r["U"][:, 0, :] - G["U_ipopt_like"][:, 0, :]).max() <= 1e-4      # the published command


def test_the_checker_reads_no_environment():
    """The CPU checker's algorithm is a function of its arguments alone: rules are varied through kmpc_opts (degen_theta, unstick, ...; defaults from
    csrc/kmpc_tuning.h), never through the process environment -- bench.py times it from pthread workers and every parity test compares against it."""
    import glob
    srcs = glob.glob(os.path.join(os.path.dirname(GOLD), os.pardir, "oracle", "*.c"))
    assert len(srcs) >= 2
    for f in srcs:
        assert "getenv" not in open(f).read(), f
