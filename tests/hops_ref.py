"""Brute-force numpy restatement of kb_sense_hops's definition (include/kilobots_hip.h), shared by the hops tests and
tools/bench_hops.py.

The graph is the range matrix of tests/reduce_ref.py (the predicate !(d2 > R2) in float32, every operation rounded on its
own); everything after it is integers: a level-by-level breadth-first search on the boolean matrix, the parent as the lowest
index one hop closer, the root along the parents.  Comparisons with the device are by equality."""
import numpy as np

from tests.reduce_ref import in_range

UNLIMITED = 1024        # KB_HOPS_UNLIMITED


def hops_env(inr, seed, max_hops=UNLIMITED):
    """One env whose range matrix is known: inr [N, N] bool (in_range), seed [N] bool or integers (non-zero = seed).
    Returns (hops, parent, root [N] int32, stats [2] int32)."""
    N = inr.shape[0]
    seed = np.asarray(seed).reshape(N) != 0
    hop = np.full(N, -1, dtype=np.int32)
    parent = np.full(N, -1, dtype=np.int32)
    root = np.full(N, -1, dtype=np.int32)
    hop[seed] = 0
    root[seed] = np.flatnonzero(seed)
    frontier, level = seed.copy(), 0
    while frontier.any() and level < max_hops:
        level += 1
        frontier = inr[frontier].any(0) & (hop < 0)
        hop[frontier] = level
    for i in np.flatnonzero(hop > 0):
        parent[i] = np.argmax(inr[i] & (hop == hop[i] - 1))     # (the first True: the lowest index)
    for level in range(1, int(hop.max(initial=-1)) + 1):
        at = hop == level
        root[at] = root[parent[at]]
    stats = np.array([(hop >= 0).sum(), hop.max(initial=-1)], dtype=np.int32)
    return hop, parent, root, stats


def restate_env(x, y, seed, R, max_hops=UNLIMITED):
    """One env: x, y [N] float32 (world units), seed [N].  Returns (hops, parent, root, stats)."""
    return hops_env(in_range(x, y, R), seed, max_hops)


def restate(x, y, seed, R, max_hops=UNLIMITED):
    """x, y [E, N] float32, seed [E, N] -> (hops, parent, root [E, N] int32, stats [E, 2] int32)."""
    envs = [restate_env(x[e], y[e], seed[e], R, max_hops) for e in range(x.shape[0])]
    return tuple(np.stack([env[k] for env in envs]) for k in range(4))


def candidates(inr, hop):
    """[N] int: how many neighbours one hop closer every kilobot has (0 for seeds and unreached ones)."""
    closer = inr & (hop[None, :] == hop[:, None] - 1) & (hop[:, None] > 0)
    return closer.sum(1)


def serpentine(n=1024):
    """A chain of n kilobots in metres, [n, 2] float64: 22 rows of 46 kilobots at pitch 0.04 m from x = -0.9, the rows 0.06 m
    apart from y = -0.66 and alternating in direction, one connector 0.03 m above the last kilobot of every row; the first
    n points.  At R = 0.045 m every kilobot is in range of its predecessor and its successor only."""
    pts = []
    for r in range(22):
        xs = -0.9 + 0.04 * np.arange(46)
        if r % 2:
            xs = xs[::-1]
        y = -0.66 + 0.06 * r
        pts += [(x, y) for x in xs]
        pts.append((xs[-1], y + 0.03))
    return np.array(pts[:n], dtype=np.float64)
