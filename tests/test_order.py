"""The ordered leader search on the device (include/kmpc_order.h): kmpc_order_fleet against the numpy order of tests/order_ref.py, and
kmpc_order_follow_fleet / kmpc_order_lane_step_fleet against the pair searches kmpc_follow_fleet / kmpc_lane_step_fleet ON THE DEVICE, which are
the specification.  Everything here is exact: the order is integers, and the ordered entry points promise the pair searches' outputs bit for bit
(compared as raw 64-bit words, so that NaN and -0.0 count); there is no tolerance anywhere in this file."""
import numpy as np
import pytest

import fleet_scenario as F
import follow_ref as FR
import lanes_ref as LR
import order_ref as OR

pytestmark = pytest.mark.gpu

# wave, workgroup (256) and sort-chunk (2048) edges; 70 001 lies beyond 2^16 and takes 35 workgroups per sort pass and 274 per lane table
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4097, 70001)
CANARY = 64


def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64).cuda()


def _lib():
    import torch
    from mkz_mpc_path_follower_amd import _lib as M
    from mkz_mpc_path_follower_amd._stage import ptr, stream
    return M, M.load(), ptr, stream(torch.device("cuda", 0))


def workspace(B, lanes_max=0):
    import ctypes as C
    import torch
    M, L, _, _ = _lib()
    n = C.c_int64()
    M.check(L.kmpc_order_bytes(B, lanes_max, C.byref(n)))
    return torch.full((n.value + CANARY,), 0x5A, dtype=torch.uint8, device="cuda"), n.value


class Fleet:
    """a draw's vehicles on the device as the loops hand them over (s and e_ct inside a [B,4] error table at columns 3 and 0, speed inside a
    [B,8] state at column 3), or contiguous (strided=False)"""

    def __init__(self, d, strided=True, use_path=True, use_present=True):
        import torch
        B = self.B = len(d["s"])
        if strided:
            err, state = np.full((B, 4), -7.0), np.full((B, 8), -7.0)
            err[:, 3], state[:, 3] = d["s"], d["v"]
            if "e_ct" in d:
                err[:, 0] = d["e_ct"]
            self.err, self.state = dev(err), dev(state)
            self.s, self.ss, self.v, self.vs, self.e, self.es = self.err[:, 3], 4, self.state[:, 3], 8, self.err[:, 0], 4
        else:
            self.s, self.ss, self.v, self.vs = dev(d["s"]), 1, dev(d["v"]), 1
            self.e, self.es = (dev(d["e_ct"]), 1) if "e_ct" in d else (None, 1)
        self.pid = dev(d["path_id"], torch.int32) if use_path and d["path_id"] is not None else None
        self.present = dev(d["present"], torch.uint8) if use_present and d["present"] is not None else None
        self.host = (d["s"], d["v"], d["path_id"] if use_path else None, d["present"] if use_present else None)

    def head(self, ptr):
        return (0, self.B, ptr(self.s), self.ss, ptr(self.v), self.vs, ptr(self.pid), ptr(self.present))

    def order(self, ws=None):
        """kmpc_order_fleet -> (order tensor [B] with a canary tail, count tensor)"""
        import torch
        M, L, ptr, st = _lib()
        buf = torch.full((self.B + CANARY,), -9, dtype=torch.int32, device="cuda")
        cnt = torch.full((1 + CANARY,), -9, dtype=torch.int32, device="cuda")
        ws, nb = workspace(self.B) if ws is None else ws
        M.check(L.kmpc_order_fleet(*self.head(ptr), ptr(buf), ptr(cnt), ptr(ws), nb, st))
        torch.cuda.synchronize()
        assert (buf[self.B:] == -9).all() and (cnt[1:] == -9).all() and (ws[nb:] == 0x5A).all()
        return buf[:self.B], cnt[:1]


def _check_order(d, what, **kw):
    f = Fleet(d, **kw)
    o, n = OR.order(*f.host)
    g, c = f.order()
    g = g.cpu().numpy()
    assert int(c.item()) == n, (what, int(c.item()), n)
    assert np.array_equal(g, o), (what, np.flatnonzero(g != o)[:8], g[:8], o[:8])


# ---------------------------------------------------------------- 1: the order
@pytest.mark.parametrize("B", SIZES)
def test_order_is_the_numpy_order(B):
    """the tie-rich draw (multiples of 0.5 m, bad vehicles, absent ones, negative path ids) and the wide draw (continuous +-1e6, path ids up to
    2^30 + 5, -0.0), with and without path_id / present, contiguous inputs: order_out and count_out equal order_ref.order exactly; the words behind
    order_out, count_out and the workspace are intact"""
    for kind in ("ties", "wide"):
        for use in (True, False):
            _check_order(OR.draw(kind, B, 0, 3), (kind, B, use), strided=False, use_path=use, use_present=use)


def test_order_of_adversarial_one_spot_and_strided_fleets():
    """B = 300: arclengths a few ulps apart around 2^52, 2^53, 1e308 with negatives and +-0.0; every vehicle of a path at one arclength; and the
    loops' own layout (the track score's err_out + 3 with stride 4, the plant's state + 3 with stride 8)"""
    for seed in range(3):
        _check_order(OR.draw("adversarial", 300, seed, 3), ("adversarial", seed), strided=False)
        _check_order(OR.draw("adversarial", 300, seed, 0), ("adversarial one path", seed), strided=False)
    _check_order(OR.draw("one_spot", 300, 0, 3), "one spot", strided=False)
    _check_order(OR.draw("one_spot", 300, 0, 0), "one spot, one path", strided=False)
    _check_order(OR.draw("ties", 300, 1, 3), "strided", strided=True)
    _check_order(OR.draw("wide", 2049, 1, 3), "strided wide", strided=True)


# ---------------------------------------------------------------- 2: the ordered follower
def bits(t):
    import torch
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def _follow_pair(f, d, stats, order=None, want=(True, True, True)):
    """kmpc_follow_fleet (order None) or kmpc_order_follow_fleet on a Fleet -> [v_out, gap, leader, stat] device tensors (None where not wanted);
    every output has a canary tail"""
    import torch
    M, L, ptr, st = _lib()
    B = f.B
    rows, cap = dev(d["rows"]), dev(d["v_cap"])
    out = torch.full((B + CANARY,), -3.0, dtype=torch.float64, device="cuda")
    gap = torch.full((B + CANARY, 2), -3.0, dtype=torch.float64, device="cuda") if want[0] else None
    leader = torch.full((B + CANARY,), -3, dtype=torch.int32, device="cuda") if want[1] else None
    stat = stats if want[2] else None
    args = f.head(ptr) + (ptr(rows), ptr(cap), ptr(out), ptr(gap), ptr(leader), ptr(stat))
    if order is None:
        M.check(L.kmpc_follow_fleet(*args, st))
    else:
        M.check(L.kmpc_order_follow_fleet(*args, ptr(order), st))
    torch.cuda.synchronize()
    for t in (out, gap, leader):
        assert t is None or (t[B:] == -3).all()
    return [out[:B], None if gap is None else gap[:B], None if leader is None else leader[:B], stat]


def _same(a, b, what):
    import torch
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(bits(x), bits(y)), (what, i, torch.nonzero(bits(x) != bits(y))[:6].flatten().tolist())


@pytest.mark.parametrize("B", SIZES)
def test_ordered_follower_is_the_pair_search(B):
    """three consecutive calls on one record each (fresh draws, stat carried through), tie-rich on three paths and wide on one path with path_id
    NULL: v_cap_out, gap_out, leader_out and every word of stat of kmpc_order_follow_fleet equal kmpc_follow_fleet's bit for bit; for B <= 2049
    the leaders and gaps are also follow_ref.follow's"""
    import torch
    from mkz_mpc_path_follower_amd.ref_traj import fresh_follow_stat
    for kind, paths in (("ties", 3), ("wide", 0), ("ties", 0)):
        sa, sb = (fresh_follow_stat(B, torch.device("cuda", 0)) for _ in range(2))
        for call in range(3):
            d = OR.draw(kind, B, call, paths)
            f = Fleet(d)
            o, _ = f.order()
            a = _follow_pair(f, d, sa)
            b = _follow_pair(f, d, sb, order=o)
            _same(a, b, (kind, B, call))
            if B <= 2049 and call == 0:
                e = FR.follow(d["s"], d["v"], d["path_id"], d["present"], d["rows"], d["v_cap"])
                assert np.array_equal(b[2].cpu().numpy(), e["leader"]) and np.array_equal(b[1][:, 0].cpu().numpy(), e["gap"])
        assert (sb[:, 0] == 3.0).all()


def test_ordered_follower_on_hard_arclengths_and_without_optional_outputs():
    """B = 300, adversarial and one-spot draws; then a NULL gap_out, leader_out and stat, one case each"""
    import torch
    from mkz_mpc_path_follower_amd.ref_traj import fresh_follow_stat
    fresh = lambda: fresh_follow_stat(300, torch.device("cuda", 0))
    for kind, paths, seed in (("adversarial", 0, 0), ("adversarial", 3, 1), ("adversarial", 0, 2), ("one_spot", 3, 0), ("one_spot", 0, 0)):
        d = OR.draw(kind, 300, seed, paths)
        f = Fleet(d)
        o, _ = f.order()
        _same(_follow_pair(f, d, fresh()), _follow_pair(f, d, fresh(), order=o), (kind, paths, seed))
    d = OR.draw("ties", 300, 4, 3)
    f = Fleet(d)
    o, _ = f.order()
    for want in ((False, True, True), (True, False, True), (True, True, False)):
        _same(_follow_pair(f, d, fresh(), want=want), _follow_pair(f, d, fresh(), order=o, want=want), want)


# ---------------------------------------------------------------- 3: the ordered lane step
def occ_dev(occ):
    import torch
    return torch.from_numpy(np.ascontiguousarray(occ, dtype=np.uint32).view(np.int32).copy()).cuda()


def populate(d, n_lanes, seed, sparse=False):
    """a lanes_ref draw's lane words redrawn for ONE n_lanes: lanes uniform in 0 ... n_lanes - 1 (sparse: one vehicle in 64 in lane 1, the rest in
    lane 0), one vehicle in ten in mid-change from a neighbouring lane (two thirds of them on the ramp, the others on the target's own bits so
    that the release can happen), e_ct within 0.7 m of the offset; the draw's junk words stay"""
    rng = np.random.default_rng(5 * len(d["s"]) + seed + 100 * n_lanes)
    B = len(d["s"])
    lr, rec = d["lane_rows"].copy(), d["rec"].copy()
    lr[:, 0] = n_lanes
    lane = (rng.random(B) < 1.0 / 64).astype(np.float64) if sparse else np.floor(rng.random(B) * n_lanes)
    rec[:, LR.LANE] = rec[:, LR.LANE_FROM] = lane
    with np.errstate(invalid="ignore"):          # the draw's junk lane rows
        rec[:, LR.OFFSET] = lane * lr[:, 1]
    if n_lanes > 1:
        mid = rng.random(B) < 0.10
        dirn = np.where(lane == 0, 1.0, np.where(lane == n_lanes - 1, -1.0, rng.choice([-1.0, 1.0], B)))
        rec[mid, LR.LANE_FROM] = (lane + dirn)[mid]
        ramp = mid & (rng.random(B) < 0.67)
        with np.errstate(invalid="ignore"):
            rec[ramp, LR.OFFSET] = (lane * lr[:, 1] + dirn * lr[:, 1] * rng.uniform(0.05, 1.0, B))[ramp]
    with np.errstate(invalid="ignore"):
        e_ct = np.where(np.isfinite(d["e_ct"]), rec[:, LR.OFFSET] + rng.uniform(-0.7, 0.7, B), d["e_ct"])
    return dict(d, lane_rows=lr, rec=rec, e_ct=e_ct, occ=LR.bit(rec[:, LR.LANE]) | LR.bit(rec[:, LR.LANE_FROM]))


def _lane_call(f, d, k, fr, lr, rec, occ_in, order=None, lanes_max=0, ws=None):
    """kmpc_lane_step_fleet (order None) or kmpc_order_lane_step_fleet -> [v_out, gap, leader, nbr, occ_out]; rec is updated in place"""
    import torch
    M, L, ptr, st = _lib()
    B = f.B
    cap = dev(d["v_cap"])
    out = torch.full((B + CANARY,), -3.0, dtype=torch.float64, device="cuda")
    gap = torch.full((B + CANARY, 2), -3.0, dtype=torch.float64, device="cuda")
    leader = torch.full((B + CANARY,), -3, dtype=torch.int32, device="cuda")
    nbr = torch.full((B + CANARY, 4, 2), -3.0, dtype=torch.float64, device="cuda")
    occ_out = torch.full((B + CANARY,), -3, dtype=torch.int32, device="cuda")
    args = (0, B, k, d["dt"], ptr(f.s), f.ss, ptr(f.e), f.es, ptr(f.v), f.vs, ptr(f.pid), ptr(f.present), ptr(fr), ptr(lr), ptr(cap), ptr(out),
            ptr(occ_in), ptr(occ_out), ptr(rec), ptr(gap), ptr(leader), ptr(nbr))
    if order is None:
        M.check(L.kmpc_lane_step_fleet(*args, st))
    else:
        M.check(L.kmpc_order_lane_step_fleet(*args, ptr(order), lanes_max, ptr(ws[0]), ws[1], st))
        torch.cuda.synchronize()
        assert (ws[0][ws[1]:] == 0x5A).all()
    torch.cuda.synchronize()
    for t in (out, gap, leader, nbr, occ_out):
        assert (t[B:] == -3).all()
    return [out[:B], gap[:B], leader[:B], nbr[:B], occ_out[:B]]


def _lane_sequence(B, n_lanes, maxes, paths=3, sparse=False, kind="ties", periods=3):
    """lanes_ref.calls' sequence -- the rows, record and occupancy of draw 0 to begin with, period k on draw k's arclengths, speeds, path ids,
    present and caps, e_ct following the running record's offset -- run through kmpc_lane_step_fleet and, for every lanes_max of `maxes`,
    through kmpc_order_lane_step_fleet, each on its own carried record and occupancy: all outputs and every word of the records equal"""
    import torch
    d0 = populate(OR.draw(kind, B, 0, paths, lanes=True), n_lanes, 0, sparse)
    fr, lr = dev(d0["follow_rows"]), dev(d0["lane_rows"])
    recs = [dev(d0["rec"]) for _ in range(1 + len(maxes))]
    occs = [occ_dev(d0["occ"]) for _ in range(1 + len(maxes))]
    spaces = [workspace(B, m) for m in maxes]
    moved = 0
    for k in range(periods):
        dk = OR.draw(kind, B, k, paths, lanes=True)
        rec_h = recs[0].cpu().numpy()
        with np.errstate(invalid="ignore"):
            e_ct = rec_h[:, LR.OFFSET] + (dk["e_ct"] - dk["rec"][:, LR.OFFSET])
        d = dict(dk, e_ct=e_ct)
        f = Fleet(d)
        o, _ = f.order(spaces[0]) if spaces else f.order()
        a = _lane_call(f, d, k, fr, lr, recs[0], occs[0])
        for i, m in enumerate(maxes):
            b = _lane_call(f, d, k, fr, lr, recs[1 + i], occs[1 + i], order=o, lanes_max=m, ws=spaces[i])
            _same(a + [recs[0]], b + [recs[1 + i]], (B, n_lanes, m, k))
            occs[1 + i] = b[4].clone()
        moved += int((recs[0][:, LR.N_CHANGES].cpu().numpy() != rec_h[:, LR.N_CHANGES]).sum())
        occs[0] = a[4].clone()
    return moved, recs[0].cpu().numpy()


@pytest.mark.parametrize("n_lanes,maxes", [(1, (1, 0)), (2, (2, 1)), (3, (3, 2, 1)), (32, (32, 5))])
def test_ordered_lane_step_is_the_pair_search(n_lanes, maxes):
    """three periods (both parities of k, vehicles in mid-change, records and occupancy carried) at every size up to 70 001: lanes_max equal to
    N_LANES (every search from the tables) and SMALLER (bands beyond the tables walk) give kmpc_lane_step_fleet's v_cap_out, occ_out, gap_out,
    leader_out, nbr_out and every word of rec, bit for bit"""
    moved = 0
    for B in SIZES:
        moved += _lane_sequence(B, n_lanes, maxes)[0]
    assert (moved > 0) == (n_lanes > 1)          # the sequences are not idle: lane changes are decided in them


def test_ordered_lane_step_sparse_lane_one_and_hard_arclengths():
    """one vehicle in 64 in lane 1 of two (the population the tables exist for) at 4097 and 70 001 on one path; adversarial and one-spot
    arclengths at 300"""
    for B in (4097, 70001):
        _lane_sequence(B, 2, (2, 1), paths=0, sparse=True)
    for kind in ("adversarial", "one_spot"):
        _lane_sequence(300, 3, (3, 1), paths=3, kind=kind)
        _lane_sequence(300, 2, (2, 0), paths=0, kind=kind)


def test_one_lane_is_the_ordered_follower_and_the_follower():
    """N_LANES == 1, lane 0, fresh occupancy and record: v_cap_out, gap_out, leader_out and words 4 ... 9 of the record of
    kmpc_order_lane_step_fleet are kmpc_follow_fleet's outputs and stat words 0 ... 5"""
    import torch
    from mkz_mpc_path_follower_amd.ref_traj import fresh_follow_stat
    B = 1025
    d = OR.draw("ties", B, 2, 3, lanes=True)
    d["lane_rows"][:, 0] = 1.0
    f = Fleet(d)
    o, _ = f.order()
    rec, occ = dev(LR.fresh_rec(B)), occ_dev(np.ones(B, dtype=np.uint32))
    fd = dict(d, rows=d["follow_rows"])
    stat = fresh_follow_stat(B, torch.device("cuda", 0))
    a = _follow_pair(f, fd, stat)
    b = _lane_call(f, d, 0, dev(d["follow_rows"]), dev(d["lane_rows"]), rec, occ, order=o, lanes_max=1, ws=workspace(B, 1))
    _same(a[:3] + [stat[:, 0:6]], b[:3] + [rec[:, 4:10]], "one lane")


# ---------------------------------------------------------------- 4: an order that is not the order
def test_a_corrupted_order_reaches_nothing_outside_the_buffers():
    """B = 300, wide draw (no ties: a search reads a few positions).  Entries set to -1, B and 2^30 and two entries swapped.  The kernels test
    every entry as (uint32)entry >= (uint32)B before it indexes anything -- a thread whose own entry fails returns, a search that meets one ends,
    the lane tables count it as an empty position -- so nothing here can fault.  Asserted: the calls return; the canaries behind every output and
    the workspace are intact (inside the helpers); the outputs of every vehicle whose position is further than 64 from a damaged one are those of
    the true order, bit for bit; the vehicles that lost their position keep the words the buffers were filled with.  Nothing about the leaders
    of the vehicles near the damage."""
    import torch
    from mkz_mpc_path_follower_amd.ref_traj import fresh_follow_stat
    B = 300
    d = populate(OR.draw("wide", B, 3, 3, lanes=True), 2, 3)
    f = Fleet(d)
    o, _ = f.order()
    bad = o.clone()
    hit = (5, 77, 150, 200, 201)
    bad[5], bad[77], bad[150] = -1, B, 2 ** 30
    bad[200], bad[201] = o[201], o[200]
    pos = np.arange(B)
    far_pos = np.all(np.abs(pos[:, None] - np.array(hit)[None, :]) > 64, axis=1)
    far = torch.as_tensor(o.cpu().numpy()[far_pos]).cuda().long()
    lost = o[[5, 77, 150]].long()
    assert far.numel() > 20
    fd = dict(d, rows=d["follow_rows"])
    fresh = lambda: fresh_follow_stat(B, torch.device("cuda", 0))
    a, b = _follow_pair(f, fd, fresh(), order=o), _follow_pair(f, fd, fresh(), order=bad)
    _same([t[far] for t in a], [t[far] for t in b], "follower, far")
    assert (b[0][lost] == -3.0).all() and (b[2][lost] == -3).all()
    fr, lr = dev(d["follow_rows"]), dev(d["lane_rows"])
    for m in (2, 0):
        ra, rb = dev(d["rec"]), dev(d["rec"])
        a = _lane_call(f, d, 0, fr, lr, ra, occ_dev(d["occ"]), order=o, lanes_max=m, ws=workspace(B, m))
        b = _lane_call(f, d, 0, fr, lr, rb, occ_dev(d["occ"]), order=bad, lanes_max=m, ws=workspace(B, m))
        _same([t[far] for t in a + [ra]], [t[far] for t in b + [rb]], ("lanes, far", m))
        assert (b[0][lost] == -3.0).all() and (b[4][lost] == -3).all() and torch.equal(bits(rb[lost]), bits(dev(d["rec"])[lost]))


# ---------------------------------------------------------------- 5: the loops
def _platoon(search, radar_rows=None, steps=150):
    import torch
    from mkz_mpc_path_follower_amd import FleetRefTrajectory
    from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop
    from mkz_mpc_path_follower_amd.ref_traj import Follower, RangeSensor, follow_params
    from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator, road_params
    c = FR.CASES["path1"]
    targets = list(c["targets"])
    B = len(targets)
    tr = F.trajectory(c["path"])
    start = FR.platoon_start(tr, c["spacing"], B)
    grt = FleetRefTrajectory([F.path_dict(c["path"])], [0] * B, traj_horizon=8, traj_dt=0.2)
    sim = VehicleSimulator(B, X0=tr[start, 4], Y0=tr[start, 5], Psi0=tr[start, 3], road=road_params(B))
    sim.state[:, 3] = torch.as_tensor(targets, dtype=torch.float64, device=sim.device)
    radar = None if radar_rows is None else RangeSensor(B, rows=dev(radar_rows), seed=5)
    fo = Follower(grt, rows=follow_params(B, **c["row"]), radar=radar, search=search)
    loop = ClosedLoop(grt, sim, N=8, target_vel=targets, follower=fo)
    out = loop.run(steps, history=True)
    torch.cuda.synchronize()
    return loop, {k: v for k, v in out.items() if isinstance(v, torch.Tensor)}


def _same_histories(a, b):
    import torch
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), k


def test_platoon_loop_is_the_same_under_both_searches():
    """the three-vehicle path1 platoon, 150 periods: every history of run(history=True) and the follower's record, bit for bit"""
    import torch
    la, a = _platoon("pairs")
    lb, b = _platoon("sorted")
    _same_histories(a, b)
    assert torch.equal(bits(la.follower.stat), bits(lb.follower.stat)) and torch.equal(la.follower.leader, lb.follower.leader)
    assert not hasattr(la.follower, "order") and lb.follower.order.shape == (3,) and lb.follower.search == "sorted"
    assert (b["v_follow"][:, 1:].cpu().numpy() < np.array([6.0, 6.0])).any()          # the stage is at work in this loop


def test_radar_loop_is_the_same_under_both_searches():
    """the platoon behind a noisy radar (tests/test_range.py's kind: sigma_r 0.5 m, 20 % dropouts, the filter on) at one seed, 100 periods: the
    radar reads gap_out and leader_out, so its record is identical"""
    import torch
    import range_ref as RG
    rows = RG.rows(3, sigma_r=0.5, p_drop=0.2, filter=1.0)
    la, a = _platoon("pairs", rows, steps=100)
    lb, b = _platoon("sorted", rows, steps=100)
    _same_histories(a, b)
    assert torch.equal(bits(la.follower.radar.rec), bits(lb.follower.radar.rec))


def test_overtaking_loop_is_the_same_under_both_searches():
    """lanes_ref.OVERTAKE (two lanes, 400 periods, both fast vehicles overtake and return): lane, offset, state and every other history and the
    lane record, bit for bit; lanes_max sized from the rows"""
    import torch
    from mkz_mpc_path_follower_amd import FleetRefTrajectory
    from mkz_mpc_path_follower_amd.closed_loop import ClosedLoop
    from mkz_mpc_path_follower_amd.ref_traj import Follower, Lanes, follow_params, lane_params
    from mkz_mpc_path_follower_amd.vehicle_sim import VehicleSimulator, road_params
    c = LR.OVERTAKE
    targets = list(c["targets"])
    B = len(targets)
    tr = F.trajectory(c["path"])
    start = FR.platoon_start(tr, c["spacing"], B)

    def run(search):
        grt = FleetRefTrajectory([F.path_dict(c["path"])], [0] * B, traj_horizon=8, traj_dt=0.2)
        sim = VehicleSimulator(B, X0=tr[start, 4], Y0=tr[start, 5], Psi0=tr[start, 3], road=road_params(B))
        sim.state[:, 3] = torch.as_tensor(targets, dtype=torch.float64, device=sim.device)
        la = Lanes(grt, follow_rows=follow_params(B), lane_rows=lane_params(B, n_lanes=c["n_lanes"]), search=search)
        loop = ClosedLoop(grt, sim, N=8, target_vel=targets, lanes=la)
        out = loop.run(c["steps"], history=True)
        torch.cuda.synchronize()
        return la, grt, {k: v for k, v in out.items() if isinstance(v, torch.Tensor)}
    la, grt, a = run("pairs")
    lb, _, b = run("sorted")
    _same_histories(a, b)
    assert torch.equal(bits(la.rec), bits(lb.rec)) and torch.equal(la.occupancy, lb.occupancy)
    assert lb.lanes_max == 2 and not hasattr(la, "order") and not hasattr(la, "lanes_max")
    assert (lb.summary()["n_changes"][1:] == 2).all() and (b["lane"].cpu().numpy().max(0)[1:] == 1.0).all()
    for cls, kw in ((Follower, dict(rows=follow_params(B))), (Lanes, dict(follow_rows=follow_params(B)))):
        with pytest.raises(ValueError):
            cls(grt, search="bogus", **kw)
    with pytest.raises(ValueError):
        Lanes(grt, follow_rows=follow_params(B), search="sorted", lanes_max=33)
