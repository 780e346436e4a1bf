"""CPU side of the latency stages: the symbols and their argument checks (no GPU needed: every check comes before the first device call), the
in-force rule j(tau, d) against a brute-force delivery timeline, the restated predict-ahead against estimator_ref.model_step, and the host
validation of VehicleSimulator(cmd_queue_depth=), SensorModel(meas_delay=, depth=) and LatencyCompensator."""
import ctypes as C

import numpy as np
import pytest

import estimator_ref as E
import latency_ref as LR

NEW = ("kmpc_sim_advance_queue", "kmpc_sense_delayed_batch", "kmpc_cmd_in_force_batch", "kmpc_predict_ahead_batch")
ARG = -1   # KMPC_ERR_ARG


def test_symbols_are_exported_and_the_abi_version_stays():
    from mkz_mpc_path_follower_amd import _lib
    L = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.kmpc_abi_version() == 8


def test_argument_checks_answer_before_any_device_call():
    from mkz_mpc_path_follower_amd import _lib
    L = _lib.load()
    p = C.c_void_p(64)   # never dereferenced: every call below is refused on the host
    q = dict(B=4, state=p, cmd=p, plant=p, delay=p, queue=p, depth=4, period=0, n=10)

    def queue(**kw):
        a = dict(q, **kw)
        return L.kmpc_sim_advance_queue(0, a["B"], a["state"], a["cmd"], a["plant"], a["delay"], a["queue"], a["depth"], a["period"], a["n"], None)
    for bad in (dict(B=-1), dict(n=-1), dict(state=None), dict(cmd=None), dict(plant=None), dict(depth=1), dict(depth=0), dict(period=-1), dict(queue=None)):
        assert queue(**bad) == ARG, bad
        assert b"kmpc_sim_advance_queue" in L.kmpc_last_error(None)
    assert queue(B=0) == 0 and queue(n=0) == 0                      # nothing to do: success without a launch
    assert queue(B=0, queue=None) == ARG and queue(n=0, depth=1) == ARG   # ... but the queue's own checks still hold

    s = dict(B=4, state=p, sensor=p, period=0, id_base=0, delay=p, ring=p, depth=3, est=p)

    def sense(**kw):
        a = dict(s, **kw)
        return L.kmpc_sense_delayed_batch(0, a["B"], a["state"], a["sensor"], 1, a["period"], a["id_base"], a["delay"], a["ring"], a["depth"], a["est"], None)
    for bad in (dict(B=-1), dict(period=-1), dict(id_base=-1), dict(state=None), dict(sensor=None), dict(est=None), dict(delay=None), dict(ring=None),
                dict(depth=0)):
        assert sense(**bad) == ARG, bad
        assert b"kmpc_sense_delayed_batch" in L.kmpc_last_error(None)
    assert sense(B=0) == 0

    c = dict(B=4, hist=p, depth=5, period=3, n=10, cd=p, md=p, max_cd=30, max_md=1, out=p, z=p, L_a=1.1, L_b=1.7)

    def in_force(**kw):
        a = dict(c, **kw)
        return L.kmpc_cmd_in_force_batch(0, a["B"], a["hist"], a["depth"], a["period"], a["n"], a["cd"], a["md"], a["max_cd"], a["max_md"], a["out"], None)

    def ahead(**kw):
        a = dict(c, **kw)
        return L.kmpc_predict_ahead_batch(0, a["B"], a["z"], a["hist"], a["depth"], a["period"], a["n"], a["cd"], a["md"], a["max_cd"], a["max_md"],
                                          a["L_a"], a["L_b"], a["out"], None)
    common = (dict(B=-1), dict(period=-1), dict(n=0), dict(max_cd=-1), dict(max_md=-1), dict(hist=None), dict(cd=None), dict(md=None), dict(out=None),
              dict(depth=4),               # 1 + ceil(30 / 10) + 1 = 5
              dict(max_cd=31),             # ceil(31 / 10) = 4: needs 6
              dict(max_md=2), dict(n=7, depth=6))   # ceil(30 / 7) = 5: needs 7
    for fn, name in ((in_force, b"kmpc_cmd_in_force_batch"), (ahead, b"kmpc_predict_ahead_batch")):
        for bad in common:
            assert fn(**bad) == ARG, (name, bad)
            assert name in L.kmpc_last_error(None)
        assert fn(B=0) == 0 and fn(B=0, depth=4) == ARG
    for bad in (dict(z=None), dict(L_a=0.0), dict(L_b=-1.0), dict(L_a=float("nan")), dict(L_b=float("inf"))):
        assert ahead(**bad) == ARG, bad


@pytest.mark.parametrize("n", [10, 7])
def test_in_force_rule_is_the_brute_force_timeline(n):
    periods = 9
    total = periods * n
    for d in range(0, 4 * n + 1):
        line = LR.timeline(periods, d, n, total)
        j = LR.in_force_period(np.arange(total), d, n)
        assert np.array_equal(np.maximum(j, -1), line), d
        assert (j[: d] < 0).all() and j[d] == 0 if d < total else True
    # the queue's split is the same rule: update `up` of period p sees period p - q - (up < r)
    for d in (0, 3, n, n + 3, 2 * n, 3 * n - 1, 3 * n):
        q, r = LR.queue_split([d], 4, n)
        for p in range(6):
            up = np.arange(n)
            assert np.array_equal(p - q[0] - (up < r[0]), LR.in_force_period(p * n + up, d, n))
    q, r = LR.queue_split([-2, 1000], 4, n)
    assert q.tolist() == [0, 3] and r.tolist() == [0, 0]


def test_in_force_command_and_its_clamps():
    rng = np.random.default_rng(3)
    cmds = rng.normal(0, 1, (8, 5, 2))
    # no delays: the filter steps over period p - 1 under the command of period p - 1
    for p in range(8):
        u = LR.cmd_in_force(cmds, p, 10, [0] * 5, [0] * 5, 35, 2)
        assert np.array_equal(u, cmds[p - 1] if p else np.zeros((5, 2)))
    # d = 25, Lm = 1 in period 6: midpoint of period 4 is update 45, (45 - 25) // 10 = 2
    assert np.array_equal(LR.cmd_in_force(cmds, 6, 10, [25] * 5, [1] * 5, 35, 2), cmds[2])
    # clamps: d into [0, max], Lm into [0, min(max, period)]
    assert np.array_equal(LR.cmd_in_force(cmds, 6, 10, [99, -4, 25, 25, 25], [1, 1, 7, -3, 1], 25, 1),
                          np.stack([cmds[2, 0], cmds[4, 1], cmds[2, 2], cmds[3, 3], cmds[2, 4]]))
    assert np.array_equal(LR.cmd_in_force(cmds, 0, 10, [0] * 5, [2] * 5, 35, 2), np.zeros((5, 2)))


def test_predict_ahead_restated():
    rng = np.random.default_rng(4)
    B = 40
    z = np.stack([rng.uniform(-500, 500, B), rng.uniform(-500, 500, B), rng.uniform(-np.pi, np.pi, B), rng.uniform(0, 20, B)], 1)
    z[:4, 3] = 0.0
    cmds = np.stack([rng.uniform(-1, 1, (8, B)), rng.uniform(-0.5, 0.5, (8, B))], 2)
    # zero delays: z bit for bit, whatever the caps
    assert np.array_equal(LR.predict_ahead(z, cmds, 5, 10, np.zeros(B, int), np.zeros(B, int), 30, 2), z)
    assert np.array_equal(LR.predict_ahead(z, cmds, 5, 10, np.full(B, -3), np.full(B, -1), 30, 2), z)
    # m updates under one constant command: m calls of the estimator's model step with h = 0.01
    const = np.broadcast_to(cmds[0], cmds.shape).copy()
    for d, Lm in ((7, 0), (30, 0), (0, 2), (25, 1)):
        got = LR.predict_ahead(z, const, 6, 10, np.full(B, d), np.full(B, Lm), 30, 2)
        exp = z.copy()
        for _ in range(Lm * 10 + d):
            exp, _ = E.model_step(exp, cmds[0], 0.01)
        assert np.array_equal(got, exp), (d, Lm)
        assert not np.array_equal(got, z)
    # a changing log: each step takes the command in force at its update (d = 25, Lm = 1, period 6: updates 50 ... 84 see periods 2, 3, 4, 5)
    got = LR.predict_ahead(z, cmds, 6, 10, np.full(B, 25), np.full(B, 1), 30, 2)
    exp = z.copy()
    for tau in range(50, 85):
        exp, _ = E.model_step(exp, cmds[(tau - 25) // 10], 0.01)
    assert np.array_equal(got, exp)
    # per-vehicle delays: every vehicle as if alone
    d, Lm = rng.integers(0, 31, B), rng.integers(0, 3, B)
    got = LR.predict_ahead(z, cmds, 6, 10, d, Lm, 30, 2)
    for b in (0, 5, 17, 39):
        assert np.array_equal(got[b], LR.predict_ahead(z[b:b + 1], cmds[:, b:b + 1], 6, 10, d[b:b + 1], Lm[b:b + 1], 30, 2)[0])
    # a non-finite input stays with its vehicle
    bad = z.copy()
    bad[3, 0] = np.nan
    out = LR.predict_ahead(bad, cmds, 6, 10, d, Lm, 30, 2)
    assert np.isnan(out[3, 0]) and np.array_equal(np.delete(out, 3, 0), np.delete(got, 3, 0))


def test_restated_queue_and_delayed_sense():
    import plant_ref as R
    rng = np.random.default_rng(5)
    B, n = 6, 10
    s0, _ = R.draw_states(rng, B, vx_range=(2.0, 10.0))
    plant = np.tile(R.DEFAULT_ROW, (B, 1))
    cmds = np.stack([rng.uniform(-1, 1, (4, B)), rng.uniform(-0.3, 0.3, (4, B))], 2)
    # depth 2, delays <= n: the held-command plant, call after call
    delay = np.array([0, 3, 10, 7, -2, 1000])
    a, b, held = s0, s0, np.zeros((B, 2))
    for p in range(4):
        a = LR.advance_queue(a, cmds, p, plant, delay, 2, n)
        b, held = R.update_plant(b, cmds[p], plant, n_updates=n, cmd_delay=delay, cmd_held=held)
        assert np.array_equal(a, b), p
    # a delay of 2 n + 5: two quiet periods first
    c = LR.advance_queue(s0, cmds, 0, plant, np.full(B, 25), 4, n)
    quiet, _ = R.update_plant(s0, np.zeros((B, 2)), plant, n_updates=n)
    assert np.array_equal(c, quiet)
    # the stale fix: truth of period - L, this period's noise
    states = rng.normal(0, 1, (5, B, 8))
    sensor = np.tile([0.2, 0.2, 0.01, 0.1, 0.1, 0.0, 0.0, 0.0], (B, 1))
    L = np.array([0, 1, 2, 9, -1, 1])
    for p in range(5):
        got = LR.sense_delayed(states, sensor, 11, p, L, 3)
        for v in range(B):
            src = max(p - min(max(L[v], 0), 2), 0)
            assert np.array_equal(got[v], R.sense(states[src, v:v + 1], sensor[v:v + 1], 11, p, id_base=v)[0])


def test_host_validation_of_the_three_classes():
    import torch
    from mkz_mpc_path_follower_amd.vehicle_sim import LatencyCompensator, SensorModel, VehicleSimulator
    for bad in (1, 0, -3, 2.0, "4", True):
        with pytest.raises(ValueError):
            VehicleSimulator(3, cmd_queue_depth=bad)
    s = SensorModel(3, meas_delay=[0, 2, 1], device="cpu")
    assert s.depth == 3 and tuple(s.truth_ring.shape) == (3, 3, 4) and s.meas_delay.dtype == torch.int32 and s.meas_delay.tolist() == [0, 2, 1]
    assert SensorModel(3, meas_delay=1, depth=5, device="cpu").depth == 5 and SensorModel(3, meas_delay=0, device="cpu").depth == 1
    assert SensorModel(3, device="cpu").meas_delay is None
    for bad in (dict(meas_delay=-1), dict(meas_delay=1.0), dict(meas_delay=[1, 2]), dict(meas_delay=[[1, 1, 1]]), dict(meas_delay=2, depth=2),
                dict(meas_delay=1, depth=2.0), dict(depth=3)):
        with pytest.raises(ValueError):
            SensorModel(3, device="cpu", **bad)
    c = LatencyCompensator(3, cmd_delay=[0, 25, 11], meas_delay=1, device="cpu")
    assert (c.depth, c.max_cmd_delay, c.max_meas_delay, c.n_updates) == (5, 25, 1, 10)
    assert tuple(c.cmd_hist.shape) == (5, 3, 2) and c.cmd_delay.tolist() == [0, 25, 11] and c.meas_delay.tolist() == [1, 1, 1]
    assert c.cmd_delay.dtype == torch.int32 and c.meas_delay.dtype == torch.int32 and not c.cmd_hist.any().item()
    assert LatencyCompensator(3, device="cpu").depth == 1 and LatencyCompensator(3, cmd_delay=30, n_updates=7, device="cpu").depth == 6
    assert LatencyCompensator(3, cmd_delay=25, meas_delay=1, depth=8, device="cpu").depth == 8
    for bad in (dict(cmd_delay=-1), dict(meas_delay=-1), dict(cmd_delay=2.5), dict(meas_delay=[1, 2]), dict(n_updates=0), dict(n_updates=2.0),
                dict(cmd_delay=25, meas_delay=1, depth=4), dict(depth=0), dict(L_a=0.0), dict(L_b=float("nan"))):
        with pytest.raises(ValueError):
            LatencyCompensator(3, device="cpu", **bad)
    c.push(torch.ones((3, 2), dtype=torch.float64), 7)
    assert c.cmd_hist[2].eq(1.0).all().item() and not c.cmd_hist[[0, 1, 3, 4]].any().item()
    for bad_cmd in (torch.ones((3, 2)), torch.ones((2, 2), dtype=torch.float64), torch.ones((3, 4), dtype=torch.float64)[:, ::2]):
        with pytest.raises(ValueError):
            c.push(bad_cmd, 0)
    with pytest.raises(ValueError):
        c.push(torch.ones((3, 2), dtype=torch.float64), -1)
    with pytest.raises(ValueError):
        c.predict(torch.ones((3, 8), dtype=torch.float64)[:, 0:4], 0)       # z must be contiguous


def test_loops_refuse_history_without_a_compensator():
    from mkz_mpc_path_follower_amd.closed_loop import _ScoredLoop

    class Sim:
        B, device = 3, "cpu"
    loop = _ScoredLoop()
    loop.B, loop.sim = 3, Sim()
    with pytest.raises(ValueError):
        loop._init_estimator(None, "history")
    with pytest.raises(ValueError):
        loop._init_estimator(None, "state")
