"""Scenes for the partner walk of the contact search (kb_step_kernel.h, "narrowphase, pass 1" and the stage pass behind it)
and for the union-find walks of the label and flatten passes.

The find pass keeps the first four partners of a kilobot packed in two registers (two 16-bit entries each) and only
counts the rest; the stage pass reads those four back and walks the candidates again for partner 4, 5, ...  So what a scene
must have is owners on both sides of the boundaries at 2 and 4 partners:

    piles        for k = 1 .. 7, k + 1 kilobots inside ONE broadphase cell (35 mm), centres within 4 mm: every pair of a pile
                 touches and the kilobot in the first slot of the cell owns all k contacts with the others, the next one
                 k - 1, ...  Owners with 3, 4, 5, 6 and 7 owned contacts exist in the first substep after planting.  The
                 piles burst in that substep: they are planted again before every launch sequence.
    chain, ring  40 kilobots 32 mm apart in a row across three dozen cells, and a closed ring of 24: one island each, whose parent
                 chains are several links long and are hooked by many threads at once.

The rest of an env is a loose lattice (pitch 45 mm, nobody touches) with the sites next to a planted kilobot left out.  Ids
are shuffled per env, so that the id order (the packed list) and the slot order (the cells) differ.

Shared by tests/test_contact_search_cpu.py (every scene has on the oracle what it is there for) and
tests/test_contact_search_gpu.py (every launch bit for bit against the oracle)."""
from types import SimpleNamespace

import numpy as np

from tests import scenes
from tests.scenes import scene_id  # noqa: F401

CELL = 0.035                    # kb_abi.hip: CELL_SIZE of the 2 x 1.5 m arena, origin at its lower left corner
XMIN, YMIN = -1.0, -0.75
DIAMETER = 0.033
PILE_SPREAD = 0.004             # centres of a pile lie within this distance of each other
PILE_KS = range(1, 8)           # pile k has k + 1 kilobots
PILE_BOTS = sum(k + 1 for k in PILE_KS)         # 35
CHAIN, RING, LINK = 40, 24, 0.032
PITCH, JITTER, CLEAR = 0.045, 0.004, 0.06       # the loose lattice; sites closer than CLEAR to a planted kilobot stay empty
OWNER_COUNTS = (3, 4, 5, 6, 7)


def cell_centre(cx, cy):
    return np.array([XMIN + (cx + 0.5) * CELL, YMIN + (cy + 0.5) * CELL])


def piles(rng):
    """[35, 2]: pile k around the centre of cell (6 + 4 k, 8), every kilobot within PILE_SPREAD / 2 of that centre"""
    out = []
    for k in PILE_KS:
        r = 0.5 * PILE_SPREAD * np.sqrt(rng.uniform(0.05, 1.0, size=k + 1))
        phi = rng.uniform(0, 2 * np.pi) + 2 * np.pi * np.arange(k + 1) / (k + 1)      # (spread around: no two centres coincide)
        out.append(cell_centre(6 + 4 * k, 8) + np.stack([r * np.cos(phi), r * np.sin(phi)], -1))
    return np.concatenate(out)


def chain_and_ring(rng):
    """[64, 2]: the row of 40 at y = 0.3 m, then the ring of 24 around (0.5, -0.3) m; 0.2 mm of jitter"""
    row = np.stack([-0.7 + LINK * np.arange(CHAIN), np.full(CHAIN, 0.3)], -1)
    rad = 0.5 * LINK / np.sin(np.pi / RING)
    phi = 2 * np.pi * np.arange(RING) / RING
    ring = np.array([0.5, -0.3]) + rad * np.stack([np.cos(phi), np.sin(phi)], -1)
    return np.concatenate([row, ring]) + rng.uniform(-0.0002, 0.0002, size=(CHAIN + RING, 2))


_S = lambda name, N, parts: SimpleNamespace(name=name, N=N, parts=parts)      # noqa: E731
SCENES = [
    _S('piles-40', 40, ('piles',)),                     # one wave
    _S('chain-ring-64', 64, ('chain',)),                # one wave
    _S('all-200', 200, ('piles', 'chain')),             # generic kernel, several waves
    _S('all-1024', 1024, ('piles', 'chain')),           # the fixed-size kernel
]
E = 2
SEEDS = (1, 2, 3)               # seed s: planted, then s single-substep launches


def planted_bots(s):
    return (PILE_BOTS if 'piles' in s.parts else 0) + (CHAIN + RING if 'chain' in s.parts else 0)


def plant(s, seed):
    """(xy [E, N, 2] metres, theta [E, N], planted [E, P] ids of the planted kilobots in the order piles, chain, ring)"""
    rng = np.random.RandomState(1000 * seed + s.N)
    gx, gy = np.meshgrid((np.arange(42) - 20.5) * PITCH, (np.arange(32) - 15.5) * PITCH)
    sites = np.stack([gx.ravel(), gy.ravel()], -1)
    xy = np.zeros((E, s.N, 2))
    P = planted_bots(s)
    ids = np.zeros((E, P), np.int64)
    for e in range(E):
        fixed = np.concatenate([piles(rng) if 'piles' in s.parts else np.zeros((0, 2)),
                                chain_and_ring(rng) if 'chain' in s.parts else np.zeros((0, 2))])
        free = sites[(np.linalg.norm(sites[:, None] - fixed[None], axis=-1) > CLEAR).all(axis=1)]
        assert P <= s.N <= P + len(free), (s.name, P, len(free))
        # the loose kilobots: the free sites nearest to the middle of the arena
        free = free[np.argsort(np.linalg.norm(free, axis=-1), kind='stable')][:s.N - P]
        pos = np.concatenate([fixed, free + rng.uniform(-JITTER, JITTER, size=free.shape)])
        perm = rng.permutation(s.N)
        xy[e, perm] = pos
        ids[e] = perm[:P]
    th = rng.uniform(-np.pi, np.pi, size=(E, s.N))
    return xy, th, ids


def actions(s, seed, k):
    return scenes.random_actions(E, s.N, seed=500 + 10 * seed + k)


def islands(ws_key, ws_cnt):
    """Sizes of the islands of one env (descending) from its packed warm-start list: entry j of owner a (owners in ascending
    id, ws_cnt[a] entries each) names the partner's id; keys from 0x10000 on are walls and objects."""
    N = len(ws_cnt)
    parent = list(range(N))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    owner = np.repeat(np.arange(N), np.asarray(ws_cnt).astype(np.int64))
    for a, key in zip(owner, np.asarray(ws_key)[:len(owner)]):
        if key < 0x10000:
            parent[find(int(a))] = find(int(key))
    return sorted((int(n) for n in np.bincount([find(a) for a in range(N)], minlength=N)), reverse=True)
