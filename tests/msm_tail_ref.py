"""Plain-integer model of the MSM bucket reduce: what the tail kernels add, pair by pair, behind the accumulate stage.
A point m G is the integer m mod r, infinity is 0 (G has prime order r, so m G is infinity exactly when m = 0 mod r). Every
addition the kernels make is filed under its stage and as one of five classes, in the order the adders test them
(XYZZ::add_body, CoopAdd::add; ec_dev.h):
    o_inf    the summand is infinity            a_inf    the accumulator is infinity
    dbl      a == b != 0                        cancel   a + b == 0
    general  everything else
Written from the contracts of msm_reduce.h (serial_reduce, tile_reduce, reduce_level1, fold_windows) and msm_engine.h
(launch_front_levels, launch_scan_tail, msm_finish), on top of msm_frontend_ref.digits; Python integers only. The model follows
the PLAIN kernels: a lane that has nothing to add makes no addition, where the cooperative twin adds infinity (o_inf) instead.
tests/test_msm_tail_ref.py checks the model against the closed form sum_j (j + 1) v_j and needs no GPU."""
from collections import Counter

import msm_frontend_ref as R
from manta_rs_amd import synth

CLASSES = ("o_inf", "a_inf", "dbl", "cancel", "general")
TAIL_WINDOW_SUMS, TAIL_X_SUMS, TAIL_TWO_LEVELS = "window_sums", "x_sums", "two_levels"
MAX_EXTRA = 8  # MsmTail::MAX_EXTRA


def classify(a, b, r):
    if b % r == 0:
        return "o_inf"
    if a % r == 0:
        return "a_inf"
    if (a - b) % r == 0:
        return "dbl"
    if (a + b) % r == 0:
        return "cancel"
    return "general"


class Census:
    """Counter of (stage, class) and of (stage, where, class) for the additions filed with a `where` (a scan step, a part)."""

    def __init__(self, r):
        self.r, self.n, self.at = r, Counter(), Counter()

    def add(self, a, b, stage, where=None):
        k = classify(a, b, self.r)
        self.n[stage, k] += 1
        if where is not None:
            self.at[stage, where, k] += 1
        return (a + b) % self.r

    def count(self, stage, cls):
        """additions of class `cls` in every stage whose name starts with `stage`"""
        return sum(v for (s, k), v in self.n.items() if s.startswith(stage) and k == cls)

    def count_at(self, stage, where, cls):
        return self.at[stage, where, cls]

    def live(self, stage, where=None):
        """additions of two points other than infinity"""
        if where is None:
            return sum(self.count(stage, k) for k in ("dbl", "cancel", "general"))
        return sum(self.at[stage, where, k] for k in ("dbl", "cancel", "general"))

    def pow2(self, a, k, stage):
        """XYZZ::dbl / HostPoint::mul_pow2: k doublings (no addition is filed)"""
        return (a << k) % self.r


def tile_reduce(cs, items, want_s, stage="tile_reduce", tile=None):
    """One tile of <= 64 items: A = sum_j X_j by a suffix scan, S = sum_j (j + 1) X_j by a tree sum of the suffix sums. `top` =
    the item count rounded up to a power of two. Additions are filed at where = (tile, "scan" | "tree", d)."""
    lim = len(items)
    assert 1 <= lim <= 64
    top = 1
    while top < lim:
        top <<= 1
    acc = list(items) + [0] * (64 - lim)
    d = 1
    while d < top:
        acc = [cs.add(acc[l], acc[l + d], stage, (tile, "scan", d)) if l + d < 64 else acc[l] for l in range(64)]
        d <<= 1
    a_out, s_out = acc[0], None
    if want_s:
        d = top >> 1
        while d >= 1:
            acc = [cs.add(acc[l], acc[l + d], stage, (tile, "tree", d)) if l < d else acc[l] for l in range(64)]
            d >>= 1
        s_out = acc[0]
    return a_out, s_out


def tiles_reduce(cs, items, want_s, stage="tile_reduce"):
    """tile_reduce over ceil(n / 64) tiles of one segment -> ([A_t], [S_t])"""
    out = [tile_reduce(cs, items[t:t + 64], want_s, stage, t // 64) for t in range(0, len(items), 64)]
    return [a for a, _ in out], [s for _, s in out]


def serial_reduce(cs, items, S, want_s, stage="serial_reduce"):
    """Every lane walks its S consecutive items from the top: acc += X_i, then sum += acc. -> ([A_t], [Sx_t]); the two chains
    are filed as stage + ".acc" and stage + ".sum"."""
    A, Sx = [], []
    for i0 in range(0, len(items), S):
        acc = tot = 0
        for x in reversed(items[i0:i0 + S]):
            acc = cs.add(acc, x, stage + ".acc")
            if want_s:
                tot = cs.add(tot, acc, stage + ".sum")
        A.append(acc)
        Sx.append(tot)
    return A, Sx


def reduce_level1(cs, A0, S0, stage="reduce_level1"):
    """(X, sumS) of 2 <= T0 <= 64 tiles: part 0 X = sum_{t >= 1} t A_t (suffix scan over lanes 1 .. T0 - 1, lane 0 cleared, tree
    sum), part 1 the tree sum of the S_t. Filed at where = (part, "scan" | "tree", d)."""
    T0 = len(A0)
    assert 2 <= T0 <= 64 and len(S0) == T0
    top = 1
    while top < T0:
        top <<= 1
    out = []
    for part in (0, 1):
        acc = [0] * 64
        if part == 0:
            acc[1:T0] = A0[1:]
            d = 1
            while d < top:
                acc = [cs.add(acc[l], acc[l + d], stage, (0, "scan", d)) if l + d < 64 else acc[l] for l in range(64)]
                d <<= 1
            acc[0] = 0
        else:
            acc[:T0] = S0
        d = top >> 1
        while d >= 1:
            acc = [cs.add(acc[l], acc[l + d], stage, (part, "tree", d)) if l < d else acc[l] for l in range(64)]
            d >>= 1
        out.append(acc[0])
    return out[0], out[1]


def front_levels(cs, buckets, segs, min_items, lgS0=2, lgS=-1, lgSP=3):
    """launch_front_levels over one window segment of `segs`: serial_reduce levels while at least min_items items are left, each
    leaving one extra point (the plain sum of its Sx: serial partial sums down to one tile, then one tile_reduce) and the A
    array, whose items from 1 on are the next level's. -> (items left for the scan tail, tail_shift, [(extra, shift)])"""
    lgS_eff = lgS if lgS >= 0 else 3
    items, shift, extras = list(buckets), 0, []
    if lgS_eff <= 0:
        return items, 0, extras
    while len(items) >= min_items and len(extras) < MAX_EXTRA:
        n = len(items)
        lg = lgS0 if segs * n >= 1 << 18 else (4 if lgS < 0 and n >= 1 << 16 else lgS_eff)
        A, Sx = serial_reduce(cs, items, 1 << lg, True)
        pin = Sx
        while len(pin) > 64:
            plg = lgSP
            while plg > 1 and (len(pin) >> plg) < 32 and len(pin) > 128:
                plg -= 1
            pin, _ = serial_reduce(cs, pin, 1 << plg, False, "serial_reduce.plain")
        extra, _ = tile_reduce(cs, pin, False, "tile_reduce.extra")
        extras.append((extra, shift))
        shift += lg
        items = A[1:]
    return items, shift, extras


def scan_tail(cs, items):
    """launch_scan_tail over what the front levels left of one segment -> (kind, staged points)"""
    T0 = -(-len(items) // 64)
    if T0 == 1:
        _, s = tile_reduce(cs, items, True, tile=0)
        return TAIL_WINDOW_SUMS, dict(win=s)
    A0, S0 = tiles_reduce(cs, items, True)
    if T0 <= 64:
        X, sumS = reduce_level1(cs, A0, S0)
        return TAIL_X_SUMS, dict(X=X, sumS=sumS)
    A1, S1 = tiles_reduce(cs, A0[1:], True, "tile_reduce.level1")
    P0, _ = tiles_reduce(cs, S0, False, "tile_reduce.sums")
    assert len(A1) == -(-(T0 - 1) // 64) and len(P0) == -(-T0 // 64)
    return TAIL_TWO_LEVELS, dict(A1=A1, S1=S1, P0=P0)


def fold(cs, kind, t, tail_shift, extras, device):
    """The window sum of one segment from its staged points: msm_finish on the host, fold_windows on the device (the same sums,
    the additions in another order)."""
    stage = "fold_windows" if device else "host_fold"
    add = lambda a, b: cs.add(a, b, stage)
    if kind == TAIL_WINDOW_SUMS:
        win = t["win"]
    elif kind == TAIL_X_SUMS:
        win = add(cs.pow2(t["X"], 6, stage), t["sumS"]) if device else add(t["sumS"], cs.pow2(t["X"], 6, stage))
    else:
        sumS = run = uA = 0
        for u in range(len(t["A1"]) - 1, -1, -1):
            sumS = add(sumS, t["S1"][u])
            if u >= 1:
                run = add(run, t["A1"][u])
                uA = add(uA, run)
        if device:
            win = cs.pow2(add(cs.pow2(uA, 6, stage), sumS), 6, stage)
            for p in t["P0"]:
                win = add(win, p)
        else:
            X = add(sumS, cs.pow2(uA, 6, stage))
            sumP = 0
            for p in t["P0"]:
                sumP = add(sumP, p)
            win = add(sumP, cs.pow2(X, 6, stage))
    if tail_shift:
        win = cs.pow2(win, tail_shift, stage)
    for x, sh in extras:
        win = add(win, cs.pow2(x, sh, stage))
    return win


def window_sum(cs, buckets, segs=1, min_items=16384, device=False):
    """front levels, scan tail and fold of one bucket window -> (window sum, tail kind)"""
    items, shift, extras = front_levels(cs, buckets, segs, min_items)
    kind, t = scan_tail(cs, items)
    return fold(cs, kind, t, shift, extras, device), kind


def closed_form(buckets, r):
    return sum((j + 1) * v for j, v in enumerate(buckets)) % r


def bucket_windows(curve, mults, scalars, c, tables):
    """The bucket arrays the accumulate and merge stages leave, as integers mod r: entry i is the point mults[i] G with the scalar
    scalars[i]. Plain bases: one array of 2^(c-1) buckets per window. Window tables: table w holds 2^(c w) P and the windows share
    ONE array."""
    r, bits = synth.FR_MODULUS[curve], synth.FR_BITS[curve]
    B, W = 1 << (c - 1), R.windows(bits, c)
    out = [[0] * B for _ in range(1 if tables else W)]
    cache = {}
    for m, k in zip(mults, scalars):
        if k not in cache:
            cache[k] = R.digits(k, r, bits, c)
        for w, mag, neg in cache[k]:
            v = -m if neg else m
            if tables:
                out[0][mag - 1] = (out[0][mag - 1] + (v << (c * w))) % r
            else:
                out[w][mag - 1] = (out[w][mag - 1] + v) % r
    return out


def msm(cs, curve, mults, scalars, c, tables, min_items=16384, device=False):
    """The whole tail of one MSM -> the result as an integer mod r: the window sums, and for plain bases the Horner chain of
    msm_finish over the windows (total = 2^c total + window, from the top)."""
    wins = bucket_windows(curve, mults, scalars, c, tables)
    sums = [window_sum(cs, b, len(wins), min_items, device)[0] for b in wins]
    total = 0
    for i, w in enumerate(reversed(sums)):
        if i:
            total = cs.pow2(total, c, "horner")
        total = cs.add(total, w, "horner")
    return total
