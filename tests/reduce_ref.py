"""Brute-force numpy restatement of kb_sense_reduce's definition (include/kilobots_hip.h), shared by the reduce tests.

float32 arrays only where the definition rounds in fp32, so every operation rounds on its own like the kernel's
(-ffp-contract=off): all pairs of an env, the predicate !(d2 > R2), the fixed-point sum in integers, min / max on the
unsigned keys of the bit patterns.  Comparisons with the device are by equality of the bit patterns."""
import numpy as np

from tests import objects_ref

SUM, MIN, MAX = 0, 1, 2
OPS = {'sum': SUM, 'min': MIN, 'max': MAX}
CLAMP = np.float32(2.0 ** 21)


def key(v):
    """uint32 keys of float32 values: unsigned order of the keys = total order of the bit patterns."""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return b ^ np.where(b >> np.uint32(31) != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def unkey(k):
    """float32 values of uint32 keys, bit pattern preserved."""
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return (k ^ np.where(k >> np.uint32(31) != 0, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(np.float32)


def quant(v, scale):
    """int32 fixed-point image of float32 values: NaN -> 0, otherwise rint(clamp(v * scale, -2^21, 2^21)), half to even."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        t = v * np.float32(scale)
    assert t.dtype == np.float32
    nan = np.isnan(t)
    q = np.rint(np.minimum(np.maximum(np.where(nan, np.float32(0), t), -CLAMP), CLAMP))
    return np.where(nan, 0, q).astype(np.int32)


def in_range(x, y, R):
    """[N, N] bool, [i, j] = kilobot j is heard by kilobot i: x, y [N] float32 world units."""
    assert x.dtype == y.dtype == np.float32
    Rw = np.float32(R) * np.float32(25)
    R2 = Rw * Rw
    ex = x[None, :] - x[:, None]
    ey = y[None, :] - y[:, None]
    d2 = ex * ex + ey * ey
    assert d2.dtype == np.float32
    inr = ~(d2 > R2)
    np.fill_diagonal(inr, False)
    return inr


def reduce_env(inr, values, op, scale=65536.0):
    """One env whose range matrix is known: inr [N, N] bool (in_range), values [N] or [N, C] float32.  Returns (out of the
    shape of values, float32; count [N] uint32)."""
    op = OPS.get(op, op)
    values = np.asarray(values)
    assert values.dtype == np.float32
    v = values.reshape(inr.shape[0], -1)
    count = inr.sum(1).astype(np.uint32)
    if op == SUM:
        # (integers below 2^31 in float64: the products and sums are exact, and the matrix product is fast)
        acc = inr.astype(np.float64) @ quant(v, scale).astype(np.float64)
        assert np.abs(acc).max(initial=0) < 2 ** 31
        out = acc.astype(np.int32).astype(np.float32) / np.float32(scale)
        assert out.dtype == np.float32
    else:
        # the keys heard by kilobot i are a run of k[cols] (np.nonzero lists the pairs row by row): one reduction per run
        k = key(v)
        cols = np.nonzero(inr)[1]
        heard = count > 0
        starts = (np.cumsum(count) - count)[heard].astype(np.intp)
        best = np.full(k.shape, 0xFFFFFFFF if op == MIN else 0, dtype=np.uint32)      # (replaced below or never looked at)
        if cols.size:
            best[heard] = (np.minimum if op == MIN else np.maximum).reduceat(k[cols], starts, axis=0)
        nothing = np.float32(np.inf if op == MIN else -np.inf).view(np.uint32)
        # (selected as integers: the bit patterns, NaN payloads included, go through untouched)
        out = np.where((count == 0)[:, None], nothing, unkey(best).view(np.uint32)).astype(np.uint32).view(np.float32)
    return out.reshape(values.shape), count


def restate_env(x, y, values, R, op, scale=65536.0):
    """One env: x, y [N] float32 (world units), values [N] or [N, C] float32.  Returns (out of the shape of values, float32;
    count [N] uint32)."""
    return reduce_env(in_range(x, y, R), values, op, scale)


def restate(x, y, values, R, op, scale=65536.0):
    """x, y [E, N], values [E, N] or [E, N, C] float32 -> (out like values, count [E, N] uint32)."""
    envs = [restate_env(x[e], y[e], values[e], R, op, scale) for e in range(x.shape[0])]
    return np.stack([o for o, _ in envs]), np.stack([c for _, c in envs])


def breadth_first(inr, root=0):
    """Hop counts [N] float32 from kilobot `root` on the range graph inr (in_range); +inf where there is no path."""
    N = inr.shape[0]
    hop = np.full(N, np.inf, dtype=np.float32)
    hop[root] = 0
    frontier, d = [root], 0
    while frontier:
        d += 1
        nxt = [j for j in np.flatnonzero(inr[frontier].any(0)) if hop[j] == np.inf]
        hop[nxt] = d
        frontier = nxt
    return hop


bits = objects_ref.bits
