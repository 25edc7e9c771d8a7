"""Numpy restatement of kb_field_step's definition (include/kilobots_hip.h), shared by the pheromone-field tests.

float32 arrays throughout, one numpy operation per rounded operation (-ffp-contract=off on the device); the deposit is an
integer sum.  The cells are those of tests/grid_ref.py (the rule of kb_sense_grid, the arena from kb_get_outline alone), the
quantisation is restated next to reduce_ref.quant with the clamp at 2^20, sine and cosine are the oracle library's sincosf as
in grid_ref.  Comparisons with the device are by equality of the bit patterns."""
import numpy as np

from tests import grid_ref
from tests import objects_ref

f32 = np.float32
SCALE = f32(65536.0)
CLAMP = f32(2.0 ** 20)
MAX_CHANNELS, MAX_ITERS = 4, 64
bits = objects_ref.bits


def quant(a):
    """int32 fixed-point image of float32 amounts: NaN -> 0, otherwise rint(clamp(a * 65536, -2^20, 2^20)), half to even
    (reduce_ref.quant with the narrower clamp: 1024 of them stay below 2^31)."""
    a = np.asarray(a, dtype=np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        t = a * SCALE
    assert t.dtype == np.float32
    nan = np.isnan(t)
    q = np.rint(np.minimum(np.maximum(np.where(nan, f32(0), t), -CLAMP), CLAMP))
    return np.where(nan, 0, q).astype(np.int32)


def per_channel(v, C):
    v = np.asarray(v, dtype=np.float32)
    return np.full(C, v, dtype=np.float32) if v.ndim == 0 else v


def deposit(flat, q, n):
    """(acc int32 [n], dep float32 [n]): the integer sum of q over the kilobots of every cell and its float image."""
    acc = np.zeros(n, dtype=np.int64)
    np.add.at(acc, flat, q.astype(np.int64))
    assert np.abs(acc).max(initial=0) < 2 ** 31
    dep = acc.astype(np.int32).astype(np.float32) / SCALE
    assert dep.dtype == np.float32
    return acc.astype(np.int32), dep


def iterate(u, keep, spread):
    """One iteration on a plane [gh, gw] float32: a neighbour outside the grid is the cell itself."""
    assert u.dtype == np.float32 and np.asarray(keep).dtype == np.float32 and np.asarray(spread).dtype == np.float32
    p = np.pad(u, 1, mode='edge')
    W, E, S, N = p[1:-1, :-2], p[1:-1, 2:], p[:-2, 1:-1], p[2:, 1:-1]
    with np.errstate(over='ignore', invalid='ignore'):
        lap = ((W + E) + (S + N)) - f32(4.0) * u
        v = u + spread * lap
        out = keep * v
    assert out.dtype == np.float32
    return out


def plane_step(F, flat, amount, keep, spread, iters):
    """One (env, channel): F [gh, gw], flat [N] cell indices, amount [N] float32 or None -> (G [gh, gw], dep [gh * gw])."""
    gh, gw = F.shape
    if amount is None:
        u, dep = F.copy(), np.zeros(gw * gh, dtype=np.float32)
    else:
        dep = deposit(flat, quant(amount), gw * gh)[1]
        u = F + dep.reshape(gh, gw)
    for _ in range(iters):
        u = iterate(u, keep, spread)
    assert u.dtype == np.float32
    return u, dep


def sense_rows(tab, G, dep, ix, iy, s, c):
    """[N, 4] float32: the rows of the kilobots in the cells (ix, iy) with sine s and cosine c on the final plane G."""
    gh, gw = G.shape
    _, _, _, _, icw, ich = grid_ref.constants(tab, gw, gh)
    hicw, hich = f32(0.5) * icw, f32(0.5) * ich
    with np.errstate(over='ignore', invalid='ignore'):
        dx = (G[iy, np.minimum(ix + 1, gw - 1)] - G[iy, np.maximum(ix - 1, 0)]) * hicw * f32(25.0)
        dy = (G[np.minimum(iy + 1, gh - 1), ix] - G[np.maximum(iy - 1, 0), ix]) * hich * f32(25.0)
        rows = np.stack([G[iy, ix], c * dx + s * dy, c * dy - s * dx, dep[iy * gw + ix]], -1)
    assert rows.dtype == np.float32
    return rows


def restate_env(tab, F, x, y, th, amount=None, keep=1.0, spread=0.0, iters=1, sense=True):
    """One env: F [C, gh, gw], x, y, th [N], amount [N, C] or None -> (G [C, gh, gw], rows [N, C, 4] or None)."""
    C, gh, gw = F.shape
    assert F.dtype == np.float32 and 1 <= C <= MAX_CHANNELS and 0 <= iters <= MAX_ITERS
    keep, spread = per_channel(keep, C), per_channel(spread, C)
    ix, iy = grid_ref.cells(tab, gw, gh, x, y)
    if sense:
        s, c = objects_ref.sincos(th, np.float32)
    G, rows = np.empty_like(F), []
    for ch in range(C):
        G[ch], dep = plane_step(F[ch], iy * gw + ix, None if amount is None else amount[:, ch], keep[ch], spread[ch], iters)
        if sense:
            rows.append(sense_rows(tab, G[ch], dep, ix, iy, s, c))
    return G, np.stack(rows, 1) if sense else None


def restate(tab, F, x, y, th, amount=None, keep=1.0, spread=0.0, iters=1, env_mask=None, sense=True, fill=None):
    """F [E, C, gh, gw], x, y, th [E, N], amount [E, N, C] (or [E, N] with one channel) or None -> (G like F, rows
    [E, N, C, 4] or None).  env_mask [E]: the envs it does not select keep their planes, and their rows are those of `fill`
    (what the output held before the call)."""
    E, C = F.shape[:2]
    if amount is not None and amount.ndim == 2:
        amount = amount[:, :, None]
    G = F.copy()
    rows = None if not sense else np.zeros(x.shape + (C, 4), dtype=np.float32) if fill is None else fill.copy()
    for e in range(E):
        if env_mask is not None and not env_mask[e]:
            continue
        G[e], r = restate_env(tab, F[e], x[e], y[e], th[e], None if amount is None else amount[e], keep, spread, iters, sense)
        if sense:
            rows[e] = r
    return G, rows
