"""Brute-force numpy restatement of kb_sense_histogram's definition (include/kilobots_hip.h), shared by the histogram tests.

float32 arrays only, so every operation rounds on its own like the kernel's (-ffp-contract=off): all pairs of an env, the
predicate !(d2 > R2), counted comparisons for ring and sector, the oracle's sincosf for the frame, the sector table read
through kb_histogram_sectors (the table the kernel is handed, not another libm's), np.bincount for the counts."""
import numpy as np

from oracle import oracle as O
from gym_kilobots_amd import _native as nat


def sector_table(n_sectors):
    """u_m, m = 1 .. n_sectors / 2 - 1, as float32 [rows, 2], through the ABI."""
    return np.array(nat.histogram_sectors(n_sectors), dtype=np.float32).reshape(-1, 2)


def ring_edges(R, n_rings):
    """(R2, [E2_1 .. E2_{n_rings - 1}]) in float32, the host side of the definition."""
    Rw = np.float32(R) * np.float32(25)
    edges = [(Rw * np.float32(r)) / np.float32(n_rings) for r in range(1, n_rings)]
    return Rw * Rw, [e * e for e in edges]


def frames(th):
    """(s, c) float32 arrays of the library's sine and cosine of every heading."""
    sc = np.array([O.sincosf(float(t)) for t in th.ravel()], dtype=np.float32).reshape(th.shape + (2,))
    return sc[..., 0], sc[..., 1]


def restate_env(x, y, th, R, n_rings, n_sectors):
    """One env: x, y, th [N] float32 (world units, radians).  Returns a dict of the intermediates, all [N, N] with
    [i, j] = kilobot j seen from kilobot i, and hist [N, n_rings, n_sectors] float32, count [N] uint32."""
    assert x.dtype == y.dtype == th.dtype == np.float32
    N = x.shape[0]
    R2, E2 = ring_edges(R, n_rings)
    ex = x[None, :] - x[:, None]
    ey = y[None, :] - y[:, None]
    d2 = ex * ex + ey * ey
    assert d2.dtype == np.float32
    inr = ~(d2 > R2)
    np.fill_diagonal(inr, False)
    ring = np.zeros((N, N), np.int64)
    for e2 in E2:
        ring += d2 > e2
    s, c = frames(th)
    a = c[:, None] * ex + s[:, None] * ey
    l = c[:, None] * ey - s[:, None] * ex
    assert a.dtype == l.dtype == np.float32
    H = n_sectors // 2
    sector = np.zeros((N, N), np.int64)
    cross = []
    if n_sectors > 1:
        low = l < 0
        a2, l2 = np.where(low, -a, a), np.where(low, -l, l)
        for u in sector_table(n_sectors):
            cr = u[0] * l2 - u[1] * a2
            assert cr.dtype == np.float32
            cross.append(cr)
            sector += cr > 0
        sector += np.where(low, H, 0)
    B = n_rings * n_sectors
    flat = (np.arange(N)[:, None] * B + ring * n_sectors + sector)[inr]
    hist = np.bincount(flat, minlength=N * B).reshape(N, n_rings, n_sectors).astype(np.float32)
    return {'d2': d2, 'inr': inr, 'ring': ring, 'sector': sector, 'a': a, 'l': l, 'cross': cross, 'E2': E2, 'R2': R2,
            'hist': hist, 'count': inr.sum(1).astype(np.uint32)}


def restate(x, y, th, R, n_rings, n_sectors):
    """x, y, th [E, N] float32 -> (hist [E, N, n_rings, n_sectors] float32, count [E, N] uint32)."""
    envs = [restate_env(x[e], y[e], th[e], R, n_rings, n_sectors) for e in range(x.shape[0])]
    return np.stack([v['hist'] for v in envs]), np.stack([v['count'] for v in envs])
