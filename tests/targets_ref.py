"""Numpy restatement of kb_sense_targets' definition (include/kilobots_hip.h), shared by the targets tests.

A brute force: the full [N, K] matrix of d2 of one env in float32 arrays, so that every operation rounds on its own like the
kernel's (-ffp-contract=off); each direction takes the least (bits of d2, index) as ONE integer key over the selected
entries of the other side, the sums are integers.  There is no compaction here, no pass and no lane: nothing of the kernel's way
to the answer.  Sine and cosine are the oracle library's sincosf.  Comparisons with the device are by equality of the bit
patterns."""
import collections

import numpy as np

from tests import objects_ref

f32 = np.float32
bits = objects_ref.bits
Targets = collections.namedtuple('Targets', ('index', 'rel', 'owner', 'dist', 'stats'))
WORLD = f32(25.0)


def slots(points_m):
    """(tx, tx) float32 world units of float32 points in metres: one multiplication each."""
    p = np.asarray(points_m)
    assert p.dtype == np.float32 and p.shape[-1] == 2
    return p[..., 0] * WORLD, p[..., 1] * WORLD


def squared(x, y, tx, ty):
    """(ex, ey, d2) [N, K] float32 of one env: ex = tx - x_b, ey = ty - y_b, d2 = ex * ex + ey * ey."""
    with np.errstate(over='ignore', invalid='ignore'):
        ex = tx[None, :] - x[:, None]
        ey = ty[None, :] - y[:, None]
        d2 = ex * ex + ey * ey
    assert ex.dtype == ey.dtype == d2.dtype == np.float32
    return ex, ey, d2


def keys(d2, axis):
    """uint64 [N, K]: bits(d2) << 32 | the index along `axis` (1: the slot t, for a kilobot's choice; 0: the kilobot b, for a
    slot's)."""
    idx = np.arange(d2.shape[axis], dtype=np.uint64)
    return (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (idx[None, :] if axis == 1 else idx[:, None])


def tolerance2(tol_m):
    """T2 of the host: Tw = tol_m * 25, T2 = Tw * Tw, in float32."""
    tw = f32(tol_m) * WORLD
    return f32(tw * tw)


def quantised(d2):
    """int64 of float32 squared distances: rint(min(d2 * 65536, 2^40)), round half to even."""
    with np.errstate(over='ignore'):
        t = np.minimum(d2 * f32(65536.0), f32(2.0 ** 40))
    assert t.dtype == np.float32
    return np.rint(t).astype(np.int64)


def sum_word(q):
    """A Chamfer word of d_stats off the quantised terms: the exact integer sum, to float32 to nearest even, two divisions."""
    acc = int(q.sum(dtype=np.int64))
    assert 0 <= acc < 2 ** 62
    return (f32(np.int64(acc)) / f32(65536.0)) / f32(625.0)


def restate_env(x, y, th, points_m, tol_m, bot_select=None, slot_select=None):
    """One env: x, y, th [N] float32 (world units, radians), points_m [K, 2] float32 metres, the selections [N] and [K] of
    anything that compares with 0 (None: all) -> Targets(index [N] int32, rel [N, 4] float32, owner [K] int32, dist [K]
    float32, stats [6] float32)."""
    assert x.dtype == y.dtype == th.dtype == np.float32
    N, K = x.shape[0], points_m.shape[0]
    bots = np.arange(N) if bot_select is None else np.flatnonzero(np.asarray(bot_select) != 0)
    slts = np.arange(K) if slot_select is None else np.flatnonzero(np.asarray(slot_select) != 0)
    index, rel = np.full(N, -1, dtype=np.int32), np.zeros((N, 4), dtype=np.float32)
    owner, dist = np.full(K, -1, dtype=np.int32), np.zeros(K, dtype=np.float32)
    stats = np.array([np.inf] * 4 + [0.0] * 2, dtype=np.float32)
    if len(bots) == 0 or len(slts) == 0:
        rel[bots, 2] = np.inf
        dist[slts] = np.inf
        return Targets(index, rel, owner, dist, stats)
    tx, ty = slots(points_m)
    ex, ey, d2 = squared(x, y, tx, ty)
    T2 = tolerance2(tol_m)
    # slot to kilobot: over the selected kilobots, for the selected slots
    k0 = keys(d2, 0)[bots][:, slts].min(0)
    own = (k0 & np.uint64(0xFFFFFFFF)).astype(np.int64)
    d2s = (k0 >> np.uint64(32)).astype(np.uint32).view(np.float32)
    owner[slts] = own
    dist[slts] = np.sqrt(d2s) / WORLD
    # kilobot to slot: over the selected slots, for the selected kilobots
    k1 = keys(d2, 1)[bots][:, slts].min(1)
    t = (k1 & np.uint64(0xFFFFFFFF)).astype(np.int64)
    d2b = (k1 >> np.uint64(32)).astype(np.uint32).view(np.float32)
    index[bots] = t
    s, c = objects_ref.sincos(th[bots], np.float32)
    bx, by = ex[bots, t], ey[bots, t]
    assert s.dtype == c.dtype == bx.dtype == np.float32
    rel[bots, 0] = (c * bx + s * by) / WORLD
    rel[bots, 1] = (c * by - s * bx) / WORLD
    rel[bots, 2] = np.sqrt(d2b) / WORLD
    rel[bots, 3] = (owner[t] == bots).astype(np.float32)
    assert dist.dtype == rel.dtype == np.float32
    stats[0] = sum_word(quantised(d2b))
    stats[1] = np.sqrt(d2b.view(np.uint32).max().view(np.float32)) / WORLD
    stats[2] = sum_word(quantised(d2s))
    stats[3] = np.sqrt(d2s.view(np.uint32).max().view(np.float32)) / WORLD
    stats[4] = f32(int((~(d2s > T2)).sum()))
    stats[5] = f32(int((~(d2b > T2)).sum()))
    return Targets(index, rel, owner, dist, stats)


def restate(x, y, th, points_m, tol_m, bot_select=None, slot_select=None):
    """x, y, th [E, N] float32, points_m [E, K, 2] or [K, 2] float32, the selections [E, N] and [E, K] or None -> Targets of
    stacked arrays: index [E, N], rel [E, N, 4], owner, dist [E, K], stats [E, 6]."""
    points_m = np.asarray(points_m)
    rows = [restate_env(x[e], y[e], th[e], points_m[e] if points_m.ndim == 3 else points_m, tol_m,
                        None if bot_select is None else bot_select[e], None if slot_select is None else slot_select[e]) for e in range(x.shape[0])]
    return Targets(*(np.stack(part) for part in zip(*rows)))
