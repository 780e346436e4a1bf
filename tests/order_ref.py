"""TEST INFRASTRUCTURE: numpy restatement of the ordered leader search (include/kmpc_order.h), written from the header's text, not from the
kernels: THE ORDER as one lexsort, the search along it with the tie rule (plain for the follower, band-masked for the lanes' five searches), and
the draws that tests/test_order_ref.py and tests/test_order.py share.  follow_ref.leaders and lanes_ref.step -- the pair searches -- are the
specification these are compared with.
"""
import numpy as np

import follow_ref as FR
import lanes_ref as LR


def order(s, v, path_id=None, present=None):
    """THE ORDER -> (order [B] int64, count): usable first by path id, arclength (-0.0 as +0.0), index DESCENDING; the others last, index ascending"""
    s, v = np.asarray(s, dtype=np.float64), np.asarray(v, dtype=np.float64)
    B = len(s)
    ok = FR.usable(s, v, path_id, present)
    pid = np.zeros(B, dtype=np.int64) if path_id is None else np.asarray(path_id, dtype=np.int64)
    idx = np.arange(B)
    with np.errstate(invalid="ignore"):
        sk = np.where(ok, s, 0.0) + 0.0            # -0.0 + 0.0 = +0.0
    # lexsort: the LAST key is the primary one
    o = np.lexsort((np.where(ok, -idx, idx), sk, np.where(ok, pid, 0), ~ok))
    return o, int(ok.sum())


def search(s, v, path_id=None, present=None, band=None, behind=False, order_=None):
    """the search along the order for every vehicle -> winner [B] (-1 = none), diff [B] (|s_j - s_b| rounded once; +inf without a winner).
    band [B,B] bool or None: band[b, j] says whether j is a candidate of b's search.  behind: towards earlier positions (BEHIND) instead of later
    ones (AHEAD).  The rule: walk the positions of b's path; a difference of +inf ends the search; the first in-band candidate sets the rounded
    difference; the winner is the lowest index among the in-band candidates of the run with that same rounded difference."""
    s, v = np.asarray(s, dtype=np.float64), np.asarray(v, dtype=np.float64)
    B = len(s)
    o, n = order(s, v, path_id, present) if order_ is None else order_
    pid = np.zeros(B, dtype=np.int64) if path_id is None else np.asarray(path_id, dtype=np.int64)
    win, diff = np.full(B, -1, dtype=np.int64), np.full(B, np.inf)
    step = -1 if behind else 1
    for q in range(n):
        b = o[q]
        bj, bd = -1, np.inf
        r = q + step
        while 0 <= r < n and pid[o[r]] == pid[b]:
            j = o[r]
            r += step
            if band is not None and not band[b, j]:
                continue
            with np.errstate(over="ignore"):
                d = abs(s[j] - s[b])
            if not d < np.inf:
                break
            if bj >= 0 and d != bd:
                break
            if bj < 0:
                bj, bd = j, d
            elif j < bj:
                bj = j
        win[b], diff[b] = bj, bd
    return win, diff


def lane_searches(d, occ=None, rec=None):
    """the five searches of one lane period on a lanes_ref draw (its record and occupancy, or the given ones) -> winners [B,5], diffs [B,5], with
    the bands of include/kmpc_lanes.h after the release of step 1; a vehicle that is not usable finds nobody"""
    s, v, e_ct, lr = d["s"], d["v"], d["e_ct"], d["lane_rows"]
    rec = d["rec"] if rec is None else rec
    occ = np.asarray(d["occ"] if occ is None else occ).astype(np.uint32)
    B = len(s)
    lane, frm, offset = rec[:, LR.LANE].copy(), rec[:, LR.LANE_FROM].copy(), rec[:, LR.OFFSET]
    with np.errstate(all="ignore"):
        release = (frm != lane) & (offset == lane * lr[:, 1]) & (np.abs(e_ct - offset) <= lr[:, 5])
        frm = np.where(release, lane, frm)
        has_left, has_right = lane + 1.0 < lr[:, 0], lane >= 1.0
        own = LR.bit(lane) | LR.bit(frm)
        lbit = np.where(has_left, LR.bit(lane + 1.0), 0).astype(np.uint32)
        rbit = np.where(has_right, LR.bit(lane - 1.0), 0).astype(np.uint32)
    o = order(s, v, d["path_id"], d["present"])
    win, dif = np.full((B, 5), -1, dtype=np.int64), np.full((B, 5), np.inf)
    for i, (mask, behind) in enumerate(((own, False), (lbit, False), (lbit, True), (rbit, False), (rbit, True))):
        band = (occ[None, :] & mask[:, None]) != 0
        win[:, i], dif[:, i] = search(s, v, d["path_id"], d["present"], band, behind, o)
    return win, dif


# ---------------------------------------------------------------- the draws
KINDS = ("ties", "wide", "adversarial", "one_spot")


def draw(kind, B, seed=0, paths=3, lanes=False):
    """a follow_ref.draw (lanes=False) or lanes_ref.draw (lanes=True) dict whose arclengths and path ids are of one of four kinds:
    ties         the module's own draw as it is: multiples of 0.5 m, exact ties
    wide         continuous arclengths in +-1e6, path ids spread up to 2^30 + 5 (where there are paths), a few -0.0
    adversarial  arclengths a few ulps apart around 2^52, 2^53, 1e308, 1 or 3, mixed with negatives of those and +-0.0: rounded differences tie
                 across distinct arclengths and overflow
    one_spot     every vehicle of a path at one arclength"""
    d = (LR.draw if lanes else FR.draw)(B, seed=seed, paths=paths)
    rng = np.random.default_rng(31 * B + 7 * seed + KINDS.index(kind))
    s = d["s"]
    good = np.isfinite(s)
    if kind == "wide":
        new = rng.uniform(-1e6, 1e6, B)
        new[rng.random(B) < 0.02] = -0.0
        if d["path_id"] is not None:
            spread = np.array([0, 1, 77, 65536, 2 ** 24 + 3, 2 ** 30 + 5], dtype=np.int64)
            pid = d["path_id"]
            d["path_id"] = np.where(pid >= 0, spread[rng.integers(0, len(spread), B)], pid).astype(np.int32)
    elif kind == "adversarial":
        base = rng.choice([2.0 ** 53, 2.0 ** 52, 1.0, 1e308, 3.0])
        new = base + np.spacing(base) * rng.integers(0, 6, B)
        neg = rng.random(B) < 0.3
        new[neg] = -rng.choice([1.0, 3.0, base, 1e308, 0.0], int(neg.sum()))
        new[rng.random(B) < 0.1] = -0.0
        new[rng.random(B) < 0.1] = 0.0
    elif kind == "one_spot":
        pid = np.zeros(B, dtype=np.int64) if d["path_id"] is None else d["path_id"].astype(np.int64)
        new = 12.5 + 100.0 * np.maximum(pid, 0)
    else:
        return d
    d["s"] = np.where(good, new, s)     # the draw's NaN and inf arclengths stay
    return d
