"""Numpy restatement of kb_sense_coverage's definition (include/kilobots_hip.h), shared by the coverage tests.

A brute force: every cell centre against every candidate, in float32 arrays so that every operation rounds on its own like
the kernel's (-ffp-contract=off); the winner is the least (bits of d2, index) taken as ONE integer key, the accumulators of
the Voronoi cells and the cost are integers.  There is no search here, no cell list and no ring: nothing of the kernel's way
to the answer.  The arena comes from kb_get_outline (objects_ref.tables), the cell centres are those of tests/grid_ref.py,
sine and cosine are the oracle library's sincosf.  Comparisons with the device are by equality of the bit patterns."""
import collections

import numpy as np

from tests import grid_ref
from tests import objects_ref

f32 = np.float32
bits = objects_ref.bits
Coverage = collections.namedtuple('Coverage', ('owner', 'dist', 'cells', 'stats'))
WORLD = f32(25.0)
CHUNK = 2048        # cell centres per block of the [centres, candidates] arrays


def keys(tab, gw, gh, x, y, cand):
    """[gh * gw, len(cand)] uint64: bits(d2) << 32 | b of every cell centre against the candidates cand (indices) of one env."""
    cx, cy = grid_ref.centres(tab, gw, gh)
    out = np.empty((gw * gh, len(cand)), dtype=np.uint64)
    with np.errstate(over='ignore', invalid='ignore'):
        for at in range(0, gw * gh, CHUNK):
            ex = x[None, cand] - cx[at:at + CHUNK, None]
            ey = y[None, cand] - cy[at:at + CHUNK, None]
            d2 = ex * ex + ey * ey
            assert d2.dtype == np.float32
            out[at:at + CHUNK] = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | cand.astype(np.uint64)[None]
    return out


def restate_env(tab, gw, gh, x, y, th, select=None):
    """One env: x, y, th [N] float32 (world units, radians), select [N] of anything that compares with 0 (None: all) ->
    Coverage(owner [gh, gw] int32, dist [gh, gw] float32, cells [N, 4] float32, stats [2] float32)."""
    assert x.dtype == y.dtype == th.dtype == np.float32
    N = x.shape[0]
    cand = np.arange(N) if select is None else np.flatnonzero(np.asarray(select) != 0)
    cells = np.zeros((N, 4), dtype=np.float32)
    if len(cand) == 0:
        return Coverage(np.full((gh, gw), -1, dtype=np.int32), np.full((gh, gw), np.inf, dtype=np.float32), cells,
                        np.full(2, np.inf, dtype=np.float32))
    best = keys(tab, gw, gh, x, y, cand).min(1)
    owner = (best & np.uint64(0xFFFFFFFF)).astype(np.int64)
    d2 = (best >> np.uint64(32)).astype(np.uint32).view(np.float32)
    dist = np.sqrt(d2) / WORLD
    assert dist.dtype == np.float32
    # the Voronoi cells: integer accumulators
    ix, iy = np.tile(np.arange(gw), gh), np.repeat(np.arange(gh), gw)
    n = np.bincount(owner, minlength=N)
    SX, SY = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    np.add.at(SX, owner, ix)
    np.add.at(SY, owner, iy)
    D = np.zeros(N, dtype=np.uint32)
    np.maximum.at(D, owner, d2.view(np.uint32))
    assert SX.max() < 2 ** 24 and SY.max() < 2 ** 24
    xmin, ymin, cw, ch, _, _ = grid_ref.constants(tab, gw, gh)
    own = np.flatnonzero(n > 0)
    nf = n[own].astype(np.float32)
    mx = xmin + ((SX[own].astype(np.float32) / nf) + f32(0.5)) * cw
    my = ymin + ((SY[own].astype(np.float32) / nf) + f32(0.5)) * ch
    dx, dy = mx - x[own], my - y[own]
    s, c = objects_ref.sincos(th[own], np.float32)
    assert s.dtype == c.dtype == dx.dtype == np.float32
    cells[own, 0] = (c * dx + s * dy) / WORLD
    cells[own, 1] = (c * dy - s * dx) / WORLD
    cells[own, 2] = nf
    cells[own, 3] = np.sqrt(D[own].view(np.float32)) / WORLD
    stats = np.array([cost_word(quantised(d2)), np.sqrt(d2.view(np.uint32).max().view(np.float32)) / WORLD], dtype=np.float32)
    return Coverage(owner.astype(np.int32).reshape(gh, gw), dist.reshape(gh, gw), cells, stats)


def quantised(d2):
    """int64 of float32 squared distances: rint(min(d2 * 65536, 2^40)), round half to even."""
    with np.errstate(over='ignore'):
        t = np.minimum(d2 * f32(65536.0), f32(2.0 ** 40))
    assert t.dtype == np.float32
    return np.rint(t).astype(np.int64)


def cost_word(q):
    """Word 0 of d_stats off the quantised terms: the exact integer sum, to float32 to nearest even, two divisions."""
    acc = int(q.sum(dtype=np.int64))
    assert abs(acc) < 2 ** 62
    return (f32(np.int64(acc)) / f32(65536.0)) / f32(625.0)


def restate(tab, gw, gh, x, y, th, select=None):
    """x, y, th [E, N] float32, select [E, N] or None -> Coverage of stacked arrays: owner, dist [E, gh, gw], cells [E, N, 4],
    stats [E, 2]."""
    rows = [restate_env(tab, gw, gh, x[e], y[e], th[e], None if select is None else select[e]) for e in range(x.shape[0])]
    return Coverage(*(np.stack(part) for part in zip(*rows)))
