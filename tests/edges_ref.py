"""The definition of kb_sense_edges (include/kilobots_hip.h), brute force in numpy, shaped like `restate` of
tests/test_neighbors_gpu.py: float32 arrays only, so that every operation rounds on its own like the kernel's
(-ffp-contract=off); all pairs of an env, the predicate !(d2 > R2), np.nonzero for ascending j, the oracle's sincosf for the
frame.  And the memory contract of the call applied to given offsets and a capacity: the expected value where the offsets
are stale."""
import numpy as np

from oracle import oracle as O
from tests import objects_ref
from tests.scenes import world  # noqa: F401

W = np.float32(25)


def in_range(x, y, R):
    """[i, j] of one env: j is a neighbour of i.  x, y [N] float32 world units.  Returns (mask, ex, ey, d2)."""
    assert x.dtype == y.dtype == np.float32
    Rw = np.float32(R) * W
    R2 = Rw * Rw
    ex = x[None, :] - x[:, None]            # [i, j] = x_j - x_i
    ey = y[None, :] - y[:, None]
    d2 = ex * ex + ey * ey
    assert ex.dtype == d2.dtype == np.float32
    inr = ~(d2 > R2)
    np.fill_diagonal(inr, False)
    return inr, ex, ey, d2


def restate_env(x, y, th, R):
    """The rows of one env: (i [n], j [n], rel [n, 4] float32, count [N] uint32), the edges ordered by (i, j)."""
    assert th.dtype == np.float32
    inr, ex, ey, d2 = in_range(x, y, R)
    i, j = np.nonzero(inr)                  # row-major: ascending i, then ascending j
    sc = np.array([O.sincosf(float(t)) for t in th], np.float32).reshape(-1, 2)
    s, c = sc[i, 0], sc[i, 1]
    exi, eyi = ex[i, j], ey[i, j]
    rel = np.empty((len(i), 4), np.float32)
    rel[:, 0] = (c * exi + s * eyi) / W
    rel[:, 1] = (c * eyi - s * exi) / W
    rel[:, 2] = np.sqrt(d2[i, j]) / W
    rel[:, 3] = th[j] - th[i]
    return i, j, rel, inr.sum(1).astype(np.uint32)


def restate(x, y, th, R):
    """The definition on x, y, th [E, N] float32 (world units).  Returns (src [nnz] int32, dst [nnz] int32, rel [nnz, 4]
    float32, count [E, N] uint32, offsets [E N + 1] int64): node e N + i for kilobot i of env e."""
    E, N = x.shape
    src, dst, rel, count = [], [], [], np.zeros((E, N), np.uint32)
    for e in range(E):
        i, j, r, count[e] = restate_env(x[e], y[e], th[e], R)
        src.append((e * N + i).astype(np.int32))
        dst.append((e * N + j).astype(np.int32))
        rel.append(r)
    offsets = np.zeros(E * N + 1, np.int64)
    np.cumsum(count.ravel(), out=offsets[1:])
    return np.concatenate(src), np.concatenate(dst), np.concatenate(rel), count, offsets


def contract(true, offsets, capacity, before):
    """What the call leaves in its outputs when it is handed `offsets` [E N + 1] (any int64 values whose rows do not overlap)
    and `capacity`.  true: (src, dst, rel, count, offsets) of restate; before: (src, dst, rel) as the buffers of `capacity`
    entries were before the call.  Row r owns [lo, hi), both clipped to [0, capacity]; it receives its first
    min(count_r, hi - lo) edges, then -1 / +0.0; nothing else changes.  Returns (src, dst, rel, owned): owned [capacity]
    bool, the slots some row owns."""
    tsrc, tdst, trel, count, toff = true
    src, dst, rel = (np.array(b, copy=True) for b in before)
    assert len(src) == len(dst) == len(rel) == capacity and len(offsets) == len(toff)
    owned = np.zeros(capacity, bool)
    clipped = np.clip(np.asarray(offsets, np.int64), 0, capacity)
    for r in range(len(toff) - 1):
        lo, hi = int(clipped[r]), int(clipped[r + 1])
        if hi <= lo:
            continue
        assert not owned[lo:hi].any(), 'rows overlap'
        owned[lo:hi] = True
        m, t0 = min(int(count.ravel()[r]), hi - lo), int(toff[r])
        src[lo:lo + m], dst[lo:lo + m], rel[lo:lo + m] = tsrc[t0:t0 + m], tdst[t0:t0 + m], trel[t0:t0 + m]
        src[lo + m:hi], dst[lo + m:hi], rel[lo + m:hi] = -1, -1, np.float32(0)
    return src, dst, rel, owned


bits = objects_ref.bits
