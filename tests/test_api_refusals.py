"""The refusals of the fleet stages' C entry points, as a table: (entry point, arguments, return code, the exact text of kmpc_last_error(NULL)).

INTEGRATION.md tells callers to read these texts, and for include/kmpc_follow.h, kmpc_lanes.h, kmpc_range.h and kmpc_order.h, the row fillers
(kmpc_*_default, kmpc_*_init) and the argument checks of the plan, profile, score, fault and wander entry points nothing else pins them.  Every text
below is a literal, written down from what the library answered before these functions were given one required-buffer helper, one argument block
per search family and one row filler.  Every argument check of these functions answers before the first HIP call (and before a path handle is
read), so the table runs without a device: no case here passes its checks with B > 0.

Where two things are wrong at once, the case names the text that must win: the order of the checks is part of the contract.
"""
import ctypes as C

import numpy as np

INF = float("inf")
ARG = -1   # KMPC_ERR_ARG
DP = C.POINTER(C.c_double)

_buf = np.zeros(64)
X = _buf.ctypes.data          # a buffer that is given: no refused call reads it
Y = X + 8 * 32                # a second one, for the pairs that must differ
NUL = None

WS3_0, WS3_4 = 2304, 3840    # kmpc_order_bytes(3, 0) and (3, 4): the workspace of three vehicles without and with four lanes' tables


def lib():
    from mkz_mpc_path_follower_amd import _lib
    return _lib.load()


def answered(cases):
    """every (name, entry point, arguments, return code, text): the call must return the code and, where it refuses, leave exactly `text` in
    kmpc_last_error(NULL); all the misses are reported together"""
    L = lib()
    bad = []
    for name, entry, args, rc, text in cases:
        got = getattr(L, entry)(*args)
        if got != rc:
            bad.append("%s: %s returned %d, expected %d (%r)" % (name, entry, got, rc, L.kmpc_last_error(None).decode()))
        elif rc != 0 and L.kmpc_last_error(None).decode() != text:
            bad.append("%s:\n  expected %r\n  got      %r" % (name, text, L.kmpc_last_error(None).decode()))
    assert not bad, "\n".join(bad)


def follow(B=3, s=X, ss=1, v=X, vs=1, rows=X, vc=X, out=X, tail=()):
    """kmpc_follow_fleet's arguments (kmpc_order_follow_fleet's with tail=(order,)); the optional buffers are never given"""
    return (0, B, s, ss, v, vs, NUL, NUL, rows, vc, out, NUL, NUL, NUL) + tuple(tail) + (NUL,)


def lane(B=3, k=0, dt=0.1, s=X, ss=1, e=X, es=1, v=X, vs=1, fr=X, lr=X, vc=X, out=X, oi=X, oo=Y, rec=X, tail=()):
    """kmpc_lane_step_fleet's arguments (kmpc_order_lane_step_fleet's with tail=(order, lanes_max, workspace, workspace_bytes))"""
    return (0, B, k, dt, s, ss, e, es, v, vs, NUL, NUL, fr, lr, vc, out, oi, oo, rec, NUL, NUL, NUL) + tuple(tail) + (NUL,)


def rng(B=3, dt=0.1, truth=X, leader=X, vt=X, vts=1, vk=X, vks=1, fr=X, rr=X, period=0, vc=X, out=X, rec=X):
    """kmpc_range_follow_batch's arguments"""
    return (0, B, dt, truth, leader, vt, vts, vk, vks, fr, rr, 0, period, 0, vc, out, rec, NUL, NUL)


def order(B=3, s=X, ss=1, v=X, vs=1, out=X, ws=X, nbytes=WS3_0):
    """kmpc_order_fleet's arguments"""
    return (0, B, s, ss, v, vs, NUL, NUL, out, X, ws, nbytes, NUL)


def test_follow_and_range_refusals():
    f, r = "kmpc_follow_fleet: ", "kmpc_range_follow_batch: "
    stride = f + "bad B / s_stride / speed_stride (B=%d, s_stride=%d, speed_stride=%d; strides >= 1)"
    rstride = r + "bad B / stride (B=%d, speed_true_stride=%d, speed_known_stride=%d; strides >= 1)"
    rnull = r + "null required buffer (truth %s, leader %s, speed_true %s, speed_known %s, follow_rows %s, range_rows %s, v_cap %s, v_cap_out %s, rec %s)"
    g, n = "given", "NULL"
    answered([
        ("follow B < 0", "kmpc_follow_fleet", follow(B=-1), ARG, stride % (-1, 1, 1)),
        ("follow s_stride", "kmpc_follow_fleet", follow(ss=0), ARG, stride % (3, 0, 1)),
        ("follow speed_stride", "kmpc_follow_fleet", follow(vs=0), ARG, stride % (3, 1, 0)),
        ("follow nulls", "kmpc_follow_fleet", follow(v=NUL, vc=NUL, out=NUL), ARG,
         f + "null required buffer (s_along given, speed NULL, rows given, v_cap NULL, v_cap_out NULL)"),
        ("follow s_along and rows", "kmpc_follow_fleet", follow(s=NUL, rows=NUL), ARG,
         f + "null required buffer (s_along NULL, speed given, rows NULL, v_cap given, v_cap_out given)"),
        ("follow: a bad stride before a NULL buffer", "kmpc_follow_fleet", follow(ss=0, s=NUL), ARG, stride % (3, 0, 1)),
        ("follow: a bad stride is refused at B = 0 too", "kmpc_follow_fleet", follow(B=0, vs=-2), ARG, stride % (0, 1, -2)),
        ("follow B = 0, nothing given", "kmpc_follow_fleet", follow(B=0, s=NUL, v=NUL, rows=NUL, vc=NUL, out=NUL), 0, None),
        ("range B < 0", "kmpc_range_follow_batch", rng(B=-2), ARG, rstride % (-2, 1, 1)),
        ("range speed_true_stride", "kmpc_range_follow_batch", rng(vts=0), ARG, rstride % (3, 0, 1)),
        ("range speed_known_stride", "kmpc_range_follow_batch", rng(vks=0), ARG, rstride % (3, 1, 0)),
        ("range dt 0", "kmpc_range_follow_batch", rng(dt=0.0), ARG, r + "dt must be finite and > 0"),
        ("range dt inf", "kmpc_range_follow_batch", rng(dt=INF), ARG, r + "dt must be finite and > 0"),
        ("range dt NaN", "kmpc_range_follow_batch", rng(dt=float("nan")), ARG, r + "dt must be finite and > 0"),
        ("range period < 0", "kmpc_range_follow_batch", rng(period=-1), ARG, r + "bad period (-1; 0 <= period < 2^61)"),
        ("range period 2^61", "kmpc_range_follow_batch", rng(period=2 ** 61), ARG, r + "bad period (2305843009213693952; 0 <= period < 2^61)"),
        ("range nulls", "kmpc_range_follow_batch", rng(leader=NUL, vk=NUL, rr=NUL, rec=NUL), ARG, rnull % (g, n, g, n, g, n, g, g, n)),
        ("range the other nulls", "kmpc_range_follow_batch", rng(truth=NUL, vt=NUL, fr=NUL, vc=NUL, out=NUL), ARG, rnull % (n, g, n, g, n, g, n, n, g)),
        ("range: a bad stride before a bad dt", "kmpc_range_follow_batch", rng(vts=0, dt=0.0), ARG, rstride % (3, 0, 1)),
        ("range: a bad dt before a bad period", "kmpc_range_follow_batch", rng(dt=-1.0, period=-1), ARG, r + "dt must be finite and > 0"),
        ("range: a bad dt before a NULL buffer", "kmpc_range_follow_batch", rng(dt=0.0, truth=NUL), ARG, r + "dt must be finite and > 0"),
        ("range: a bad period before a NULL buffer", "kmpc_range_follow_batch", rng(period=-5, rec=NUL), ARG, r + "bad period (-5; 0 <= period < 2^61)"),
        ("range: a bad dt is refused at B = 0 too", "kmpc_range_follow_batch", rng(B=0, dt=0.0), ARG, r + "dt must be finite and > 0"),
        ("range B = 0, nothing given", "kmpc_range_follow_batch",
         rng(B=0, truth=NUL, leader=NUL, vt=NUL, vk=NUL, fr=NUL, rr=NUL, vc=NUL, out=NUL, rec=NUL), 0, None),
    ])


def test_lane_refusals():
    s, o = "kmpc_lane_step_fleet: ", "kmpc_ref_offset_batch: "
    stride = s + "bad B / k / stride (B=%d, k=%d, s_stride=%d, e_stride=%d, speed_stride=%d; strides >= 1)"
    null = s + ("null required buffer (s_along %s, e_ct %s, speed %s, follow_rows %s, lane_rows %s, v_cap %s, v_cap_out %s, occ_in %s, occ_out %s, "
                "rec %s)")
    same = s + "occ_in == occ_out (the occupancy every vehicle reads is a snapshot nobody writes)"
    obad = o + "bad B / H1 / offset_stride (B=%d, H1=%d, >= 1, B * H1 < 2^31; offset_stride=%d, >= 1)"
    g, n = "given", "NULL"
    answered([
        ("lane B < 0", "kmpc_lane_step_fleet", lane(B=-1), ARG, stride % (-1, 0, 1, 1, 1)),
        ("lane k < 0", "kmpc_lane_step_fleet", lane(k=-1), ARG, stride % (3, -1, 1, 1, 1)),
        ("lane s_stride", "kmpc_lane_step_fleet", lane(ss=0), ARG, stride % (3, 0, 0, 1, 1)),
        ("lane e_stride", "kmpc_lane_step_fleet", lane(es=0), ARG, stride % (3, 0, 1, 0, 1)),
        ("lane speed_stride", "kmpc_lane_step_fleet", lane(vs=0), ARG, stride % (3, 0, 1, 1, 0)),
        ("lane dt 0", "kmpc_lane_step_fleet", lane(dt=0.0), ARG, s + "dt must be finite and > 0"),
        ("lane dt inf", "kmpc_lane_step_fleet", lane(dt=INF), ARG, s + "dt must be finite and > 0"),
        ("lane nulls", "kmpc_lane_step_fleet", lane(e=NUL, fr=NUL, vc=NUL, oi=NUL, rec=NUL), ARG, null % (g, n, g, n, g, n, g, n, g, n)),
        ("lane the other nulls", "kmpc_lane_step_fleet", lane(s=NUL, v=NUL, lr=NUL, out=NUL, oo=NUL), ARG, null % (n, g, n, g, n, g, n, g, n, g)),
        ("lane occ_in == occ_out", "kmpc_lane_step_fleet", lane(oi=X, oo=X), ARG, same),
        ("lane: a bad stride before a bad dt", "kmpc_lane_step_fleet", lane(es=0, dt=0.0), ARG, stride % (3, 0, 1, 0, 1)),
        ("lane: a bad stride before a NULL buffer", "kmpc_lane_step_fleet", lane(ss=0, s=NUL), ARG, stride % (3, 0, 0, 1, 1)),
        ("lane: a bad dt before a NULL buffer", "kmpc_lane_step_fleet", lane(dt=-0.1, rec=NUL), ARG, s + "dt must be finite and > 0"),
        ("lane: a NULL elsewhere before occ_in == occ_out", "kmpc_lane_step_fleet", lane(oi=X, oo=X, rec=NUL), ARG,
         null % (g, g, g, g, g, g, g, g, g, n)),
        ("lane: both occupancies NULL is a NULL buffer", "kmpc_lane_step_fleet", lane(oi=NUL, oo=NUL), ARG, null % (g, g, g, g, g, g, g, n, n, g)),
        ("lane: a bad dt is refused at B = 0 too", "kmpc_lane_step_fleet", lane(B=0, dt=0.0), ARG, s + "dt must be finite and > 0"),
        ("lane B = 0, occ_in == occ_out and nothing else given", "kmpc_lane_step_fleet",
         lane(B=0, s=NUL, e=NUL, v=NUL, fr=NUL, lr=NUL, vc=NUL, out=NUL, oi=X, oo=X, rec=NUL), 0, None),
        ("offset B < 0", "kmpc_ref_offset_batch", (0, -1, 9, X, X, 16, NUL), ARG, obad % (-1, 9, 16)),
        ("offset H1 0", "kmpc_ref_offset_batch", (0, 3, 0, X, X, 16, NUL), ARG, obad % (3, 0, 16)),
        ("offset stride 0", "kmpc_ref_offset_batch", (0, 3, 9, X, X, 0, NUL), ARG, obad % (3, 9, 0)),
        ("offset B * H1 at 2^31", "kmpc_ref_offset_batch", (0, 65536, 32768, X, X, 1, NUL), ARG, obad % (65536, 32768, 1)),
        ("offset ref NULL", "kmpc_ref_offset_batch", (0, 3, 9, NUL, X, 16, NUL), ARG, o + "null required buffer (ref NULL, offset given)"),
        ("offset offset NULL", "kmpc_ref_offset_batch", (0, 3, 9, X, NUL, 16, NUL), ARG, o + "null required buffer (ref given, offset NULL)"),
        ("offset: a bad H1 before a NULL buffer", "kmpc_ref_offset_batch", (0, 3, 0, NUL, NUL, 16, NUL), ARG, obad % (3, 0, 16)),
        ("offset: a bad H1 is refused at B = 0 too", "kmpc_ref_offset_batch", (0, 0, 0, NUL, NUL, 16, NUL), ARG, obad % (0, 0, 16)),
        ("offset B = 0, nothing given", "kmpc_ref_offset_batch", (0, 0, 9, NUL, NUL, 1, NUL), 0, None),
    ])


def test_order_refusals():
    n64 = C.c_int64(-1)
    b, f, fo, ln = "kmpc_order_bytes: ", "kmpc_order_fleet: ", "kmpc_order_follow_fleet: ", "kmpc_order_lane_step_fleet: "
    bbad = b + "bad argument (B=%d, lanes_max=%d (0 ... 32), bytes_out %s)"
    stride = "bad B / s_stride / speed_stride (B=%d, s_stride=%d, speed_stride=%d; strides >= 1)"
    short = f + "workspace_bytes %d < kmpc_order_bytes(%d, 0) = %d"
    fnull = f + "null required buffer (s_along %s, speed %s, order_out %s, workspace %s)"
    fonull = fo + "null required buffer (s_along %s, speed %s, rows %s, v_cap %s, v_cap_out %s, order %s)"
    lstride = ln + "bad B / k / stride (B=%d, k=%d, s_stride=%d, e_stride=%d, speed_stride=%d; strides >= 1)"
    lshort = ln + "workspace_bytes %d < kmpc_order_bytes(%d, %d) = %d"
    lnull = ln + ("null required buffer (s_along %s, e_ct %s, speed %s, follow_rows %s, lane_rows %s, v_cap %s, v_cap_out %s, occ_in %s, occ_out %s, "
                  "rec %s, order %s, workspace %s)")
    same = ln + "occ_in == occ_out (the occupancy every vehicle reads is a snapshot nobody writes)"
    g, n = "given", "NULL"
    tail = lambda order=X, lanes_max=4, ws=X, nbytes=WS3_4: (order, lanes_max, ws, nbytes)
    answered([
        ("bytes B < 0", "kmpc_order_bytes", (-1, 0, C.byref(n64)), ARG, bbad % (-1, 0, g)),
        ("bytes lanes_max < 0", "kmpc_order_bytes", (3, -1, C.byref(n64)), ARG, bbad % (3, -1, g)),
        ("bytes lanes_max 33", "kmpc_order_bytes", (3, 33, C.byref(n64)), ARG, bbad % (3, 33, g)),
        ("bytes out NULL", "kmpc_order_bytes", (3, 0, NUL), ARG, bbad % (3, 0, n)),
        ("order B < 0", "kmpc_order_fleet", order(B=-1), ARG, f + stride % (-1, 1, 1)),
        ("order s_stride", "kmpc_order_fleet", order(ss=0), ARG, f + stride % (3, 0, 1)),
        ("order speed_stride", "kmpc_order_fleet", order(vs=0), ARG, f + stride % (3, 1, 0)),
        ("order short workspace", "kmpc_order_fleet", order(nbytes=WS3_0 - 1), ARG, short % (WS3_0 - 1, 3, WS3_0)),
        ("order nulls", "kmpc_order_fleet", order(v=NUL, ws=NUL), ARG, fnull % (g, n, g, n)),
        ("order the other nulls", "kmpc_order_fleet", order(s=NUL, out=NUL), ARG, fnull % (n, g, n, g)),
        ("order: a bad stride before a short workspace", "kmpc_order_fleet", order(ss=0, nbytes=0), ARG, f + stride % (3, 0, 1)),
        ("order: a short workspace before a NULL buffer", "kmpc_order_fleet", order(s=NUL, nbytes=16), ARG, short % (16, 3, WS3_0)),
        ("order: a negative size at B = 0 is a short workspace", "kmpc_order_fleet", order(B=0, nbytes=-1), ARG, short % (-1, 0, 0)),
        ("order B = 0, nothing given", "kmpc_order_fleet", order(B=0, s=NUL, v=NUL, out=NUL, ws=NUL, nbytes=0), 0, None),
        ("order follow B < 0", "kmpc_order_follow_fleet", follow(B=-1, tail=(X,)), ARG, fo + stride % (-1, 1, 1)),
        ("order follow s_stride", "kmpc_order_follow_fleet", follow(ss=0, tail=(X,)), ARG, fo + stride % (3, 0, 1)),
        ("order follow order NULL", "kmpc_order_follow_fleet", follow(tail=(NUL,)), ARG, fonull % (g, g, g, g, g, n)),
        ("order follow nulls", "kmpc_order_follow_fleet", follow(s=NUL, rows=NUL, out=NUL, tail=(X,)), ARG, fonull % (n, g, n, g, n, g)),
        ("order follow the other nulls", "kmpc_order_follow_fleet", follow(v=NUL, vc=NUL, tail=(X,)), ARG, fonull % (g, n, g, n, g, g)),
        ("order follow: a bad stride before a NULL buffer", "kmpc_order_follow_fleet", follow(vs=0, tail=(NUL,)), ARG, fo + stride % (3, 1, 0)),
        ("order follow B = 0, nothing given", "kmpc_order_follow_fleet",
         follow(B=0, s=NUL, v=NUL, rows=NUL, vc=NUL, out=NUL, tail=(NUL,)), 0, None),
        ("order lane B < 0", "kmpc_order_lane_step_fleet", lane(B=-1, tail=tail()), ARG, lstride % (-1, 0, 1, 1, 1)),
        ("order lane k < 0", "kmpc_order_lane_step_fleet", lane(k=-3, tail=tail()), ARG, lstride % (3, -3, 1, 1, 1)),
        ("order lane e_stride", "kmpc_order_lane_step_fleet", lane(es=0, tail=tail()), ARG, lstride % (3, 0, 1, 0, 1)),
        ("order lane dt", "kmpc_order_lane_step_fleet", lane(dt=0.0, tail=tail()), ARG, ln + "dt must be finite and > 0"),
        ("order lane lanes_max < 0", "kmpc_order_lane_step_fleet", lane(tail=tail(lanes_max=-1)), ARG, ln + "lanes_max -1 outside 0 ... 32"),
        ("order lane lanes_max 33", "kmpc_order_lane_step_fleet", lane(tail=tail(lanes_max=33)), ARG, ln + "lanes_max 33 outside 0 ... 32"),
        ("order lane short workspace", "kmpc_order_lane_step_fleet", lane(tail=tail(nbytes=WS3_4 - 1)), ARG, lshort % (WS3_4 - 1, 3, 4, WS3_4)),
        ("order lane nulls", "kmpc_order_lane_step_fleet", lane(e=NUL, fr=NUL, vc=NUL, oi=NUL, rec=NUL, tail=tail(ws=NUL)), ARG,
         lnull % (g, n, g, n, g, n, g, n, g, n, g, n)),
        ("order lane the other nulls", "kmpc_order_lane_step_fleet", lane(s=NUL, v=NUL, lr=NUL, out=NUL, oo=NUL, tail=tail(order=NUL)), ARG,
         lnull % (n, g, n, g, n, g, n, g, n, g, n, g)),
        ("order lane occ_in == occ_out", "kmpc_order_lane_step_fleet", lane(oi=X, oo=X, tail=tail()), ARG, same),
        ("order lane: a bad stride before a bad dt", "kmpc_order_lane_step_fleet", lane(ss=0, dt=0.0, tail=tail()), ARG, lstride % (3, 0, 0, 1, 1)),
        ("order lane: a bad dt before lanes_max", "kmpc_order_lane_step_fleet", lane(dt=0.0, tail=tail(lanes_max=33)), ARG,
         ln + "dt must be finite and > 0"),
        ("order lane: a bad dt before a NULL buffer", "kmpc_order_lane_step_fleet", lane(dt=0.0, s=NUL, tail=tail()), ARG, ln + "dt must be finite and > 0"),
        ("order lane: lanes_max out of range before a short workspace", "kmpc_order_lane_step_fleet", lane(tail=tail(lanes_max=40, nbytes=0)), ARG,
         ln + "lanes_max 40 outside 0 ... 32"),
        ("order lane: a short workspace before a NULL buffer", "kmpc_order_lane_step_fleet", lane(rec=NUL, tail=tail(order=NUL, nbytes=8)), ARG,
         lshort % (8, 3, 4, WS3_4)),
        ("order lane: a NULL elsewhere before occ_in == occ_out", "kmpc_order_lane_step_fleet", lane(oi=X, oo=X, tail=tail(order=NUL)), ARG,
         lnull % (g, g, g, g, g, g, g, g, g, g, n, g)),
        ("order lane: lanes_max is refused at B = 0 too", "kmpc_order_lane_step_fleet", lane(B=0, tail=tail(lanes_max=33)), ARG,
         ln + "lanes_max 33 outside 0 ... 32"),
        ("order lane B = 0, occ_in == occ_out and nothing else given", "kmpc_order_lane_step_fleet",
         lane(B=0, s=NUL, e=NUL, v=NUL, fr=NUL, lr=NUL, vc=NUL, out=NUL, oi=X, oo=X, rec=NUL, tail=tail(order=NUL, lanes_max=0, ws=NUL, nbytes=0)),
         0, None),
    ])
    L = lib()
    for B, lanes_max, nbytes in ((3, 0, WS3_0), (3, 4, WS3_4), (0, 0, 0)):   # the sizes the texts above quote
        assert L.kmpc_order_bytes(B, lanes_max, C.byref(n64)) == 0 and n64.value == nbytes, (B, lanes_max, n64.value)


def test_handle_entry_points_refuse_before_the_handle_is_read():
    """the plan, profile and score entry points: a NULL handle answers first, and every later argument check answers before the handle is read
    (H is a given handle that is no path set: nothing here gets as far as reading it)"""
    H = X
    plan = lambda ps=H, B=3, kappa=X, state=X, stride=8, pid=X, vc=X, rows=X, out=X: (ps, B, kappa, state, stride, pid, vc, rows, out, NUL, NUL, NUL)
    prof = lambda ps=H, B=3, kappa=X, table=X, state=X, stride=8, pid=X, vc=X, rows=X, out=X: \
        (ps, B, kappa, table, state, stride, pid, vc, rows, out, NUL, NUL, NUL)
    road = lambda ps=H, B=3, table=X, state=X, stride=8, pid=X, base=X, out=Y: (ps, B, table, state, stride, pid, base, out, NUL, NUL)
    batch = lambda p=H, B=3, state=X, stride=8, tol=0.5, status=NUL, iters=NUL, cmd=NUL, latch=NUL: \
        (p, B, state, stride, tol, status, iters, cmd, latch, NUL, NUL, NUL, NUL, NUL)
    fleet = lambda p=H, B=3, state=X, stride=8, pid=X, tol=0.5, status=NUL, iters=NUL, cmd=NUL, latch=NUL: \
        (p, B, state, stride, pid, tol, status, iters, cmd, latch, NUL, NUL, NUL, NUL, NUL)
    bad = "%s: bad B / state_stride (B=%d, state_stride=%d; state_stride >= %d)"
    cases = []
    for fn, args in (("kmpc_speed_plan_fleet", plan), ("kmpc_speed_plan_fleet_profile", prof), ("kmpc_road_profile_fleet", road)):
        cases += [
            (fn + " handle", fn, args(ps=NUL), ARG, fn + ": null path set"),
            (fn + ": a NULL handle before everything else", fn, args(ps=NUL, B=-1, stride=0, state=NUL), ARG, fn + ": null path set"),
            (fn + " B < 0", fn, args(B=-1), ARG, bad % (fn, -1, 8, 2)),
            (fn + " stride", fn, args(stride=1), ARG, bad % (fn, 3, 1, 2)),
            (fn + " state NULL", fn, args(state=NUL), ARG, fn + ": null required buffer"),
            (fn + " path_id NULL", fn, args(pid=NUL), ARG, fn + ": null required buffer"),
            (fn + ": a bad stride before a NULL buffer", fn, args(stride=1, state=NUL), ARG, bad % (fn, 3, 1, 2)),
        ]
    cases += [
        ("plan kappa NULL", "kmpc_speed_plan_fleet", plan(kappa=NUL), ARG, "kmpc_speed_plan_fleet: null required buffer"),
        ("plan v_plan_out NULL", "kmpc_speed_plan_fleet", plan(out=NUL), ARG, "kmpc_speed_plan_fleet: null required buffer"),
        ("plan B = 0, nothing given", "kmpc_speed_plan_fleet", plan(B=0, kappa=NUL, state=NUL, pid=NUL, vc=NUL, rows=NUL, out=NUL), 0, None),
        ("plan with a map: the map NULL", "kmpc_speed_plan_fleet_profile", prof(table=NUL), ARG, "kmpc_speed_plan_fleet_profile: null required buffer"),
        ("plan with a map B = 0, nothing given", "kmpc_speed_plan_fleet_profile",
         prof(B=0, kappa=NUL, table=NUL, state=NUL, pid=NUL, vc=NUL, rows=NUL, out=NUL), 0, None),
        ("road profile NULL", "kmpc_road_profile_fleet", road(table=NUL), ARG, "kmpc_road_profile_fleet: null required buffer"),
        ("road road_out == road_base", "kmpc_road_profile_fleet", road(base=X, out=X), ARG,
         "kmpc_road_profile_fleet: road_out must not be road_base (the scaling would compound call after call)"),
        ("road: a NULL buffer before road_out == road_base", "kmpc_road_profile_fleet", road(state=NUL, base=X, out=X), ARG,
         "kmpc_road_profile_fleet: null required buffer"),
        ("road: road_out == road_base is refused at B = 0 too", "kmpc_road_profile_fleet", road(B=0, base=X, out=X), ARG,
         "kmpc_road_profile_fleet: road_out must not be road_base (the scaling would compound call after call)"),
        ("road B = 0, nothing given", "kmpc_road_profile_fleet", road(B=0, table=NUL, state=NUL, pid=NUL, base=NUL, out=NUL), 0, None),
    ]
    for fn, args in (("kmpc_track_score_batch", batch), ("kmpc_track_score_fleet", fleet)):
        together = fn + ": status, iters, cmd and stop_latch are given all together or all NULL"
        cases += [
            (fn + " handle", fn, args(p=NUL), ARG, fn + ": null path handle"),
            (fn + ": a NULL handle before everything else", fn, args(p=NUL, B=-1, stride=0, tol=-1.0), ARG, fn + ": null path handle"),
            (fn + " B < 0", fn, args(B=-1), ARG, bad % (fn, -1, 8, 3)),
            (fn + " stride", fn, args(stride=2), ARG, bad % (fn, 3, 2, 3)),
            (fn + " settle_tol < 0", fn, args(tol=-0.5), ARG, fn + ": settle_tol must be finite and >= 0"),
            (fn + " settle_tol inf", fn, args(tol=INF), ARG, fn + ": settle_tol must be finite and >= 0"),
            (fn + " one of the four", fn, args(status=X), ARG, together),
            (fn + " three of the four", fn, args(status=X, iters=X, cmd=X), ARG, together),
            (fn + " state NULL", fn, args(state=NUL), ARG, fn + ": null required buffer"),
            (fn + ": a bad stride before settle_tol", fn, args(stride=2, tol=-1.0), ARG, bad % (fn, 3, 2, 3)),
            (fn + ": settle_tol before the four", fn, args(tol=-1.0, latch=X), ARG, fn + ": settle_tol must be finite and >= 0"),
            (fn + ": the four before a NULL buffer", fn, args(state=NUL, cmd=X), ARG, together),
            (fn + " B = 0, nothing given", fn, args(B=0, state=NUL), 0, None),
        ]
    cases += [
        ("score fleet path_id NULL", "kmpc_track_score_fleet", fleet(pid=NUL), ARG, "kmpc_track_score_fleet: null required buffer"),
        ("score fleet B = 0, no path_id", "kmpc_track_score_fleet", fleet(B=0, state=NUL, pid=NUL), 0, None),
    ]
    answered(cases)


def test_fault_and_wander_refusals():
    s, w = "kmpc_sense_faults_batch: ", "kmpc_wander_batch: "
    sense = lambda B=3, state=X, sensor=X, faults=X, period=0, id_base=0, delay=NUL, ring=NUL, depth=0, rec=X, z=X, held=X: \
        (0, B, state, sensor, faults, 0, period, id_base, delay, ring, depth, rec, z, held, NUL, NUL, NUL)
    wander = lambda B=3, rows=X, rec=X, period=0, id_base=0, sb=NUL, so=NUL, rb=NUL, ro=NUL: (0, B, rows, rec, 0, period, id_base, sb, so, rb, ro, NUL)
    sbad = s + "bad argument (B=%d, period=%d, id_base=%d; state, sensor, faults, fault_rec, z_out and held_out are required)"
    pair = s + "meas_delay and truth_ring go together (meas_delay %s, truth_ring %s)"
    wbad = w + "bad argument (B=%d, period=%d, below 2^62; id_base=%d; wander %s, wander_rec %s)"
    wpair = w + "a base and its out go together (sensor_base %s, sensor_out %s, road_base %s, road_out %s)"
    comp = w + "an out must not be its base (the sum would compound call after call)"
    g, n = "given", "NULL"
    answered([
        ("sense B < 0", "kmpc_sense_faults_batch", sense(B=-1), ARG, sbad % (-1, 0, 0)),
        ("sense period < 0", "kmpc_sense_faults_batch", sense(period=-1), ARG, sbad % (3, -1, 0)),
        ("sense id_base < 0", "kmpc_sense_faults_batch", sense(id_base=-7), ARG, sbad % (3, 0, -7)),
        ("sense state NULL", "kmpc_sense_faults_batch", sense(state=NUL), ARG, sbad % (3, 0, 0)),
        ("sense faults NULL", "kmpc_sense_faults_batch", sense(faults=NUL), ARG, sbad % (3, 0, 0)),
        ("sense held_out NULL", "kmpc_sense_faults_batch", sense(held=NUL), ARG, sbad % (3, 0, 0)),
        ("sense delay without ring", "kmpc_sense_faults_batch", sense(delay=X, depth=2), ARG, pair % (g, n)),
        ("sense ring without delay", "kmpc_sense_faults_batch", sense(ring=X, depth=2), ARG, pair % (n, g)),
        ("sense ring depth 0", "kmpc_sense_faults_batch", sense(delay=X, ring=X, depth=0), ARG, s + "bad ring (depth=0, at least 1)"),
        ("sense: a NULL buffer before the pair", "kmpc_sense_faults_batch", sense(z=NUL, delay=X), ARG, sbad % (3, 0, 0)),
        ("sense: the pair before the depth", "kmpc_sense_faults_batch", sense(delay=X, depth=0), ARG, pair % (g, n)),
        ("sense: the pair is refused at B = 0 too", "kmpc_sense_faults_batch", sense(B=0, ring=X), ARG, pair % (n, g)),
        ("sense: the depth is refused at B = 0 too", "kmpc_sense_faults_batch", sense(B=0, delay=X, ring=X, depth=-1), ARG,
         s + "bad ring (depth=-1, at least 1)"),
        ("sense B = 0, nothing given", "kmpc_sense_faults_batch", sense(B=0, state=NUL, sensor=NUL, faults=NUL, rec=NUL, z=NUL, held=NUL), 0, None),
        ("wander B < 0", "kmpc_wander_batch", wander(B=-1), ARG, wbad % (-1, 0, 0, g, g)),
        ("wander period < 0", "kmpc_wander_batch", wander(period=-1), ARG, wbad % (3, -1, 0, g, g)),
        ("wander period 2^62", "kmpc_wander_batch", wander(period=2 ** 62), ARG, wbad % (3, 2 ** 62, 0, g, g)),
        ("wander id_base < 0", "kmpc_wander_batch", wander(id_base=-1), ARG, wbad % (3, 0, -1, g, g)),
        ("wander rows NULL", "kmpc_wander_batch", wander(rows=NUL), ARG, wbad % (3, 0, 0, n, g)),
        ("wander rec NULL", "kmpc_wander_batch", wander(rec=NUL), ARG, wbad % (3, 0, 0, g, n)),
        ("wander sensor_base alone", "kmpc_wander_batch", wander(sb=X), ARG, wpair % (g, n, n, n)),
        ("wander road_out alone", "kmpc_wander_batch", wander(sb=X, so=Y, ro=X), ARG, wpair % (g, g, n, g)),
        ("wander sensor_out is sensor_base", "kmpc_wander_batch", wander(sb=X, so=X), ARG, comp),
        ("wander road_out is road_base", "kmpc_wander_batch", wander(sb=X, so=Y, rb=Y, ro=Y), ARG, comp),
        ("wander: a NULL buffer before a pair", "kmpc_wander_batch", wander(rec=NUL, rb=X), ARG, wbad % (3, 0, 0, g, n)),
        ("wander: a pair before out == base", "kmpc_wander_batch", wander(sb=X, so=X, rb=X), ARG, wpair % (g, g, g, n)),
        ("wander: a pair is refused at B = 0 too", "kmpc_wander_batch", wander(B=0, rows=NUL, rec=NUL, so=X), ARG, wpair % (n, g, n, n)),
        ("wander B = 0, nothing given", "kmpc_wander_batch", wander(B=0, rows=NUL, rec=NUL), 0, None),
    ])


# (filler, words, the refusal's tail behind "bad argument (", the words that are not zero): the library's defaults, word for word
FILLERS = [
    ("kmpc_track_score_init", 16, "B=%d)", {15: -1.0}),
    ("kmpc_speed_plan_default", 8, "B=%d)", {0: 2.0, 1: 0.7, 2: 1.0}),
    ("kmpc_follow_default", 8, "B=%d)", {0: 5.0, 1: 1.0, 2: 0.7, 3: 0.5, 4: 4.9}),
    ("kmpc_follow_stat_init", 8, "B=%d)", {4: INF}),
    ("kmpc_lane_default", 8, "B=%d)", {0: 1.0, 1: 3.5, 2: 1.0, 3: 0.5, 4: 20.0, 5: 0.5, 6: 1.0}),
    ("kmpc_lane_rec_init", 16, "B=%d)", {8: INF}),
    ("kmpc_range_default", 16, "B=%d)", {0: 120.0, 1: 0.25, 2: 0.12, 5: 1.0, 6: 5.0, 7: 0.01, 8: 0.25, 9: 0.0625, 10: 0.0144}),
    ("kmpc_range_rec_init", 16, "B=%d)", {5: -1.0}),
    ("kmpc_road_profile_default", 8, "n=%d)", {0: 1.0, 3: INF}),
    ("kmpc_sense_faults_default", 16, "B=%d, rows %s)", {3: 1.0, 4: 1.0, 5: 1.0, 14: INF}),
    ("kmpc_wander_default", 24, "B=%d, rows %s)", {}),
]


def test_row_fillers():
    """B < 0, a NULL with B > 0, and two filled rows against the literal defaults (the second row catches a stride mistake, the NaN row behind
    them a filler that writes past n rows)"""
    L = lib()
    cases = []
    for fn, words, tail, _ in FILLERS:
        text = fn + ": bad argument (" + tail
        says_rows = "rows" in tail
        cases += [
            (fn + " B < 0", fn, (_buf.ctypes.data_as(DP), -1), ARG, text % ((-1, "given") if says_rows else -1)),
            (fn + " NULL", fn, (NUL, 2), ARG, text % ((2, "NULL") if says_rows else 2)),
            (fn + " B < 0 and NULL", fn, (NUL, -3), ARG, text % ((-3, "NULL") if says_rows else -3)),
            (fn + " B = 0, NULL", fn, (NUL, 0), 0, None),
        ]
    answered(cases)
    for fn, words, _, nonzero in FILLERS:
        row = [nonzero.get(i, 0.0) for i in range(words)]
        got = np.full((3, words), np.nan)
        assert getattr(L, fn)(got.ctypes.data_as(DP), 2) == 0, fn
        assert got[:2].tolist() == [row, row], (fn, got[:2].tolist())
        assert np.isnan(got[2]).all(), fn
