"""Brute-force numpy restatement of kb_sense_clusters's definition (include/kilobots_hip.h), shared by the clusters tests and
tools/bench_clusters.py.

The graph is the range matrix of tests/reduce_ref.py (the predicate !(d2 > R2) in float32, every operation rounded on its
own) between the selected kilobots; labels, sizes and stats are integers: a breadth-first search on the boolean matrix from
the lowest index that has no label yet.  The table is float32 / int64 arithmetic in the order the header gives.  Comparisons
with the device are by equality, of integers and of float bit patterns."""
import numpy as np

from tests.reduce_ref import in_range

SCALE = np.float32(65536.0)
CLAMP = np.float32(2.0 ** 40)
WORLD = np.float32(25.0)


def quant(v):
    """int64 fixed-point image of float32 coordinates: rint(max(min(v * 65536, 2^40), -2^40)), half to even."""
    v = np.asarray(v, dtype=np.float32)
    t = v * SCALE
    assert t.dtype == np.float32
    return np.rint(np.maximum(np.minimum(t, CLAMP), -CLAMP)).astype(np.int64)


def labels_env(inr, select=None):
    """[N] int32: the lowest index of every selected kilobot's component on the range matrix inr (in_range), -1 for the others."""
    N = inr.shape[0]
    sel = np.ones(N, dtype=bool) if select is None else np.asarray(select).reshape(N) != 0
    m = inr & sel[:, None] & sel[None, :]
    label = np.full(N, -1, dtype=np.int32)
    todo = sel.copy()
    while todo.any():
        r = int(np.argmax(todo))        # (the first True: the lowest index without a label)
        comp = np.zeros(N, dtype=bool)
        comp[r] = True
        frontier = comp.copy()
        while frontier.any():
            frontier = m[frontier].any(0) & ~comp
            comp |= frontier
        label[comp] = r
        todo &= ~comp
    return label


def centroid(S, n):
    out = (np.float32(np.int64(S)) / np.float32(n)) / SCALE
    assert out.dtype == np.float32
    return out


def clusters_env(inr, x, y, select=None):
    """One env whose range matrix is known: x, y [N] float32 (world units).  Returns (label [N] int32, size [N] int32, table
    [N, 4] float32, stats [4] int32)."""
    assert x.dtype == y.dtype == np.float32
    N = inr.shape[0]
    label = labels_env(inr, select)
    roots = np.flatnonzero(label == np.arange(N))
    count = np.bincount(label[label >= 0], minlength=N).astype(np.int32)
    size = np.where(label >= 0, count[np.maximum(label, 0)], 0).astype(np.int32)
    table = np.zeros((N, 4), dtype=np.float32)
    qx, qy = quant(x), quant(y)
    for r in roots:
        mem = label == r
        n = int(mem.sum())
        cxw, cyw = centroid(qx[mem].sum(dtype=np.int64), n), centroid(qy[mem].sum(dtype=np.int64), n)
        ex, ey = x[mem] - cxw, y[mem] - cyw
        d2 = ex * ex + ey * ey
        assert d2.dtype == np.float32
        D = d2.view(np.uint32).max().view(np.float32)
        table[r] = (np.float32(n), cxw / WORLD, cyw / WORLD, np.sqrt(D) / WORLD)
    stats = np.array([0, 0, -1, 0], dtype=np.int32)
    if len(roots):
        sizes = count[roots]
        stats[:] = (len(roots), sizes.max(), roots[np.argmax(sizes)], (sizes == 1).sum())       # (argmax: the first, i.e. the lowest label)
    return label, size, table, stats


def restate_env(x, y, R, select=None):
    """One env: x, y [N] float32 (world units), select [N] or None.  Returns (label, size, table, stats)."""
    return clusters_env(in_range(x, y, R), x, y, select)


def restate(x, y, R, select=None):
    """x, y [E, N] float32, select [E, N] or None -> (label, size [E, N] int32, table [E, N, 4] float32, stats [E, 4] int32)."""
    envs = [restate_env(x[e], y[e], R, None if select is None else select[e]) for e in range(x.shape[0])]
    return tuple(np.stack([env[k] for env in envs]) for k in range(4))
