"""The timing tools' shared method (tools/_timing.py), as far as it can be checked without a device: the median, the order in which rotate() takes
its cases, what say() + finish() write, and that the scattered starts are the ones the tools drew inline before the method moved into one place --
the profiles under profiles/ were taken on those inputs."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import _timing as T  # noqa: E402


def test_med_odd_and_even():
    assert T.med([3.0, 1.0, 2.0]) == (2.0, 1.0, 3.0)
    assert T.med([5.0]) == (5.0, 5.0, 5.0)
    assert T.med([4.0, 1.0, 3.0, 2.0]) == (3.0, 1.0, 4.0)      # even count: the upper of the two middle values
    assert T.med([2.0, 1.0]) == (2.0, 1.0, 2.0)


def test_rotate_takes_the_cases_in_rotation():
    calls, rounds = [], []

    def timer(fn, reps):
        calls.append((fn(), reps))
        return float(len(calls))
    cases = {"a": (lambda: "a", 7), "b": (lambda: "b", 200), "c": (lambda: "c", 5)}
    res = T.rotate(cases, repeats=4, timer=timer, before=lambda: rounds.append(len(calls)))
    assert calls == [("a", 7), ("b", 200), ("c", 5)] * 4
    assert rounds == [0, 3, 6, 9]                                # before() opens every round
    assert list(res) == ["a", "b", "c"]
    assert res == {"a": [1.0, 4.0, 7.0, 10.0], "b": [2.0, 5.0, 8.0, 11.0], "c": [3.0, 6.0, 9.0, 12.0]}
    calls.clear()
    assert {k: len(v) for k, v in T.rotate(cases, timer=timer).items()} == {"a": 5, "b": 5, "c": 5} and T.REPEATS == 5


def test_say_and_finish(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(T, "LINES", [])
    monkeypatch.chdir(tmp_path)
    said = ["first line", "   B = 4096     12.5 [    12.1,     13.0]", ""]
    for s in said:
        T.say(s)
    assert capsys.readouterr().out == "".join(s + "\n" for s in said)
    T.finish(["tool.py"])
    assert os.listdir(tmp_path) == []                            # no argv[1]: nothing is written
    out = tmp_path / "out.txt"
    T.finish(["tool.py", str(out)])
    assert out.read_text() == "first line\n   B = 4096     12.5 [    12.1,     13.0]\n\n"
    assert os.listdir(tmp_path) == ["out.txt"]


def path1_trajectory():
    from mkz_mpc_path_follower_amd.ref_traj import path_arrays   # numpy alone: the [M,7] array GPSRefTrajectory keeps, without the device
    d = np.load(os.path.join(ROOT, "tests", "golden", "path1_decimated.npz"))
    return np.column_stack(path_arrays(d["t"], d["lat"], d["lon"], d["psi"], float(d["lat0"]), float(d["lon0"])))


def test_scatter_reproduces_the_inline_draws():
    tr, B = path1_trajectory(), 64
    assert tr.shape == (len(tr), 7) and len(tr) > 2 * B
    # the four lines every single-path loops() had
    rng = np.random.default_rng(2)
    idx = rng.integers(0, int(0.5 * len(tr)), B)
    X0, Y0, P0 = tr[idx, 4] + rng.uniform(-0.5, 0.5, B), tr[idx, 5] + rng.uniform(-0.5, 0.5, B), tr[idx, 3] + rng.uniform(-0.05, 0.05, B)
    after = rng.uniform(0.8, 1.3, B)                             # what plant_timing.py draws next from the same generator
    rng = np.random.default_rng(2)
    start = T.scatter(tr, B, rng)
    assert start.shape == (B, 3)
    for got, want in zip(start.T, (X0, Y0, P0)):
        assert got.tobytes() == want.tobytes()
    assert rng.uniform(0.8, 1.3, B).tobytes() == after.tobytes()


def test_scatter_variants_keep_their_draw_order():
    tr, n = path1_trajectory(), 64
    # the poses() of the fleet tools: first 60 %, 1 m, 1 m, 0.2 rad
    rng = np.random.default_rng(1)
    idx = rng.integers(0, int(0.6 * len(tr)), n)
    want = np.stack([tr[idx, 4] + rng.uniform(-1, 1, n), tr[idx, 5] + rng.uniform(-1, 1, n), tr[idx, 3] + rng.uniform(-0.2, 0.2, n)], 1)
    assert T.scatter(tr, n, np.random.default_rng(1), 0.6, (1.0, 1.0, 0.2)).tobytes() == want.tobytes()
    # the dense fleet: the sample's heading as it is, and NO draw for it -- the speeds come next from the same generator
    rng = np.random.default_rng(1)
    idx = rng.integers(0, int(0.6 * len(tr)), n)
    want = np.stack([tr[idx, 4] + rng.uniform(-1, 1, n), tr[idx, 5] + rng.uniform(-1, 1, n), tr[idx, 3]], 1)
    speeds = rng.uniform(2.0, 8.0, n)
    rng = np.random.default_rng(1)
    assert T.scatter(tr, n, rng, 0.6, (1.0, 1.0, 0.0)).tobytes() == want.tobytes()
    assert rng.uniform(2.0, 8.0, n).tobytes() == speeds.tobytes()
    # path by path, in the order of the paths
    pid = np.arange(n) % 3
    trs = [tr, tr[::2], tr[::3]]
    rng = np.random.default_rng(1)
    want = np.empty((n, 3))
    for p, t in enumerate(trs):
        sel = np.where(pid == p)[0]
        idx = rng.integers(0, int(0.6 * len(t)), len(sel))
        want[sel] = np.stack([t[idx, 4] + rng.uniform(-1, 1, len(sel)), t[idx, 5] + rng.uniform(-1, 1, len(sel)), t[idx, 3] + rng.uniform(-0.2, 0.2, len(sel))], 1)
    assert T.scatter_fleet(trs, pid, np.random.default_rng(1)).tobytes() == want.tobytes()
