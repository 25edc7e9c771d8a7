"""Numpy restatement of kb_sense_assign's definition (include/kilobots_hip.h), shared by the assign tests.

walk_env is the definition of the matching M taken literally: every admissible pair of the env, sorted by (bits of d2, b, t),
taken iff neither end has been taken.  There is no round, no choice and no rescan in it: nothing of the kernel's way to the
answer.  rounds_env is the definition of R taken literally, on the full [N, K] matrix, every entry choosing anew in every
round; it also yields a matching, which tests/test_assign_cpu.py holds against the walk's.  Both are built on
targets_ref.squared, keys and quantised, so d2 is the float32 of the kernel bit for bit.  Comparisons with the device are by
equality of the bit patterns."""
import numpy as np

from tests import objects_ref
from tests import targets_ref as TR

f32 = np.float32
bits = TR.bits
Targets = TR.Targets
WORLD = TR.WORLD
NOKEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def cutoff2(cutoff_m):
    """C2 of the host: Cw = cutoff_m * 25, C2 = Cw * Cw, in float32; None is +inf."""
    with np.errstate(over='ignore'):
        cw = f32(np.inf if cutoff_m is None else cutoff_m) * WORLD
        return f32(cw * cw)


def sides(N, K, bot_select, slot_select):
    """(selected kilobots, selected slots) as index arrays."""
    bots = np.arange(N) if bot_select is None else np.flatnonzero(np.asarray(bot_select) != 0)
    slts = np.arange(K) if slot_select is None else np.flatnonzero(np.asarray(slot_select) != 0)
    return bots, slts


def admissible(d2, bots, slts, C2):
    """bool [N, K]: both ends selected and !(d2 > C2)."""
    adm = np.zeros(d2.shape, dtype=bool)
    adm[np.ix_(bots, slts)] = True
    return adm & ~(d2 > C2)


def walk_pairs(d2, adm):
    """The matching M as (b [m], t [m]) in the order the walk takes the pairs: ascending (bits of d2, b, t)."""
    b, t = np.nonzero(adm)
    order = np.lexsort((t, b, bits(d2[b, t])))
    bot_free, slot_free = np.ones(d2.shape[0], dtype=bool), np.ones(d2.shape[1], dtype=bool)
    left = min(len(np.unique(b)), len(np.unique(t)))
    mb, mt = [], []
    for pb, pt in zip(b[order].tolist(), t[order].tolist()):
        if bot_free[pb] and slot_free[pt]:
            bot_free[pb] = slot_free[pt] = False
            mb.append(pb)
            mt.append(pt)
            left -= 1
            if left == 0:       # (every kilobot or every slot that has an admissible pair is taken: no later pair can be)
                break
    return np.array(mb, dtype=np.int64), np.array(mt, dtype=np.int64)


def rounds_env(d2, adm):
    """(R, b [m], t [m]): the round process of the definition.  In every round every unmatched kilobot chooses the least
    (bits of d2, t) among its admissible unmatched slots, every unmatched slot the least (bits of d2, b), and the pairs
    that choose each other are matched; R counts the rounds that began with an admissible pair left."""
    kt, kb = TR.keys(d2, 1), TR.keys(d2, 0)
    low = np.uint64(0xFFFFFFFF)
    left = adm.copy()
    R, mb, mt = 0, [], []
    while left.any():
        R += 1
        cb = np.where(left, kt, NOKEY).min(1)       # per kilobot
        cs = np.where(left, kb, NOKEY).min(0)       # per slot
        b = np.flatnonzero(cb != NOKEY)
        t = (cb[b] & low).astype(np.int64)
        mutual = (cs[t] & low).astype(np.int64) == b
        assert mutual.any()
        b, t = b[mutual], t[mutual]
        left[b, :] = False
        left[:, t] = False
        mb.append(b)
        mt.append(t)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    return R, cat(mb), cat(mt)


def restate_env(x, y, th, points_m, tol_m, cutoff_m=None, bot_select=None, slot_select=None, matching=None):
    """One env: x, y, th [N] float32 (world units, radians), points_m [K, 2] float32 metres -> Targets(index [N] int32, rel
    [N, 4] float32, owner [K] int32, dist [K] float32, stats [6] float32) of kb_sense_assign.  M is the walk's; R is the round
    process's.  matching: 'rounds' takes M from the round process instead (for the comparison of the two)."""
    assert x.dtype == y.dtype == th.dtype == np.float32
    N, K = x.shape[0], points_m.shape[0]
    bots, slts = sides(N, K, bot_select, slot_select)
    index, rel = np.full(N, -1, dtype=np.int32), np.zeros((N, 4), dtype=np.float32)
    owner, dist = np.full(K, -1, dtype=np.int32), np.zeros(K, dtype=np.float32)
    stats = np.zeros(6, dtype=np.float32)
    rel[bots, 2] = np.inf
    dist[slts] = np.inf
    tx, ty = TR.slots(points_m)
    ex, ey, d2 = TR.squared(x, y, tx, ty)
    adm = admissible(d2, bots, slts, cutoff2(cutoff_m))
    R, rb, rt = rounds_env(d2, adm)
    b, t = (rb, rt) if matching == 'rounds' else walk_pairs(d2, adm)
    if len(b) == 0:
        assert R == 0
        return Targets(index, rel, owner, dist, stats)
    d2m = d2[b, t]
    with np.errstate(over='ignore'):
        dm = np.sqrt(d2m) / WORLD
    s, c = objects_ref.sincos(th[b], np.float32)
    bx, by = ex[b, t], ey[b, t]
    assert s.dtype == c.dtype == bx.dtype == dm.dtype == np.float32
    index[b] = t
    rel[b, 0] = (c * bx + s * by) / WORLD
    rel[b, 1] = (c * by - s * bx) / WORLD
    rel[b, 2] = dm
    rel[b, 3] = 1.0
    owner[t] = b
    dist[t] = dm
    stats[0] = TR.sum_word(TR.quantised(d2m))
    stats[1] = np.sqrt(bits(d2m).max().view(np.float32)) / WORLD
    stats[2] = f32(np.int64(int(TR.quantised(dm).sum(dtype=np.int64)))) / f32(65536.0)
    stats[3] = f32(R)
    stats[4] = f32(int((~(d2m > TR.tolerance2(tol_m))).sum()))
    stats[5] = f32(len(b))
    return Targets(index, rel, owner, dist, stats)


def restate(x, y, th, points_m, tol_m, cutoff_m=None, bot_select=None, slot_select=None, matching=None):
    """x, y, th [E, N] float32, points_m [E, K, 2] or [K, 2] float32, the selections [E, N] and [E, K] or None -> Targets of
    stacked arrays: index [E, N], rel [E, N, 4], owner, dist [E, K], stats [E, 6]."""
    points_m = np.asarray(points_m)
    rows = [restate_env(x[e], y[e], th[e], points_m[e] if points_m.ndim == 3 else points_m, tol_m, cutoff_m,
                        None if bot_select is None else bot_select[e], None if slot_select is None else slot_select[e], matching)
            for e in range(x.shape[0])]
    return Targets(*(np.stack(part) for part in zip(*rows)))
