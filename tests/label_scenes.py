"""Scenes for the label pass of the kernels without objects (kb_step_kernel.h, "narrowphase, pass 3") and the flatten pass
behind it: per contact the lookup of last substep's impulse in the packed list of its owner -- or, where the pair changed
owner, of its partner --, the rank base of its (cell, direction) group, and the island hooking.

With the staged contacts and the previous list in LDS the pass takes the first four keys of both lists in one batch and goes
on in a loop for longer lists, sums the counters of the owner's cell-mates in front of it, and walks both roots side by side
from parents it read before the lookups.  So what a scene must have is

    long lists      owners with more than four entries in the previous list (the loop behind the batch), next to short ones
    full cells      broadphase cells (35 mm) holding three or more kilobots: rank bases over two and more cell-mates
    owner changes   pairs whose owner in one substep is the partner of the substep before: the hit comes from the second list
    islands         islands of two dozen bodies and more: root walks of several links, hooks that contend
    walls           kilobots that stay on a wall for several substeps: the one-list lookups

and it must stay where the batched code runs: no more contacts than the LDS staging area holds, status 0.

    cluster-1024    (fixed-size kernel) a 32 x 32 lattice, pitch 45 mm, shifted by -0.2 m in x; kilobots 16 i + 3, i = 0 .. 60, are
                    taken out of it into a hexagonal cluster (rings 0 .. 4) of spacing 19 mm around (0.80, 0): every kilobot
                    of it overlaps up to twelve others, the cluster bursts over the following substeps
    chains-1024     (fixed-size kernel) a row of 64 touching kilobots (pitch 32 mm) across the arena's diagonal, a closed ring
                    of 24, and eight kilobots pressed against the lower wall, one of them in the corner; the rest on the
                    free sites of a loose lattice
    cluster-200     (generic kernel of several waves, hashed bins, the volatile read form) rings 0 .. 3 of the cluster among
                    163 kilobots of the lattice

Ids of the planted kilobots are spread over the id range, so that the id order (the packed list) and the slot order (the cells)
differ.  Shared by tests/test_label_pass_cpu.py (every scene has on the oracle what it is there for) and
tests/test_label_pass_gpu.py (every launch bit for bit against the oracle)."""
from types import SimpleNamespace

import numpy as np

from tests import scenes
from tests.scenes import scene_id  # noqa: F401

CELL = 0.035                    # kb_abi.hip: CELL_SIZE of the 2 x 1.5 m arena, origin at its lower left corner
XMIN, YMIN = -1.0, -0.75
GW, GH = 58, 43                 # cells of the arena
WALL_KEY = 0x10000              # keys of the packed list from here on are walls (and objects)
E = 2
SINGLE_SUBSTEPS, FUSED_SUBSTEPS = 8, 10
PITCH = 0.045
SPACING = 0.019                 # of the hexagonal cluster: first and second neighbours overlap (19 mm, 32.9 mm < 33 mm)
ROW, RING, LINK = 64, 24, 0.032
WALL_BOTS = 8
LONG_LIST = 4                   # entries of a list that the first batch of keys covers
BATCHED_KEYS_SUBSTEPS = 3       # substeps in which a scene with 'long lists' must show them
ISLAND = 24

_S = lambda name, N, rings, chains, has: SimpleNamespace(name=name, N=N, rings=rings, chains=chains, has=has)      # noqa: E731
SCENES = [
    _S('cluster-1024', 1024, 4, False, ('long lists', 'full cells', 'owner changes', 'islands')),
    _S('chains-1024', 1024, -1, True, ('islands', 'walls')),
    _S('cluster-200', 200, 3, False, ('long lists', 'owner changes', 'islands')),      # (its cluster thins out below three per cell: no claim on its cells)
]


def hexagon(rings):
    """[1 + 3 rings (rings + 1), 2]: the sites of a hexagonal lattice of unit spacing within `rings` rings of the origin,
    ring by ring"""
    out = []
    for q in range(-rings, rings + 1):
        for r in range(-rings, rings + 1):
            ring = max(abs(q), abs(r), abs(q + r))
            if ring <= rings:
                out.append((ring, q + 0.5 * r, r * np.sqrt(3.0) / 2))
    out.sort(key=lambda t: t[0])
    return np.array([(x, y) for _, x, y in out])


def row_ring_walls():
    """[64 + 24 + 8, 2]: the row along the diagonal through the middle of the arena, the ring around (0.6, -0.4), the wall
    kilobots 1.5 mm inside the lower wall's skin from x = -0.9 on (pitch 40 mm) with the last one moved into the corner"""
    d = np.array([0.8, 0.6])
    row = (np.arange(ROW) - 0.5 * (ROW - 1))[:, None] * LINK * d[None]
    rad = 0.5 * LINK / np.sin(np.pi / RING)
    phi = 2 * np.pi * np.arange(RING) / RING
    ring = np.array([0.6, -0.4]) + rad * np.stack([np.cos(phi), np.sin(phi)], -1)
    wall = np.stack([-0.9 + 0.04 * np.arange(WALL_BOTS), np.full(WALL_BOTS, -0.75 + 0.015)], -1)
    wall[-1] = (-1.0 + 0.015, -0.75 + 0.015)
    return np.concatenate([row, ring, wall])


def plant(s):
    """(xy [E, N, 2] metres, theta [E, N]); the envs differ in their headings and in 0.2 mm of jitter"""
    rng = np.random.RandomState(4000 + s.N + (1 if s.chains else 0))
    side = int(np.ceil(np.sqrt(s.N)))
    idx = np.arange(s.N)
    xy = np.zeros((E, s.N, 2))
    if s.chains:
        fixed = row_ring_walls()
        gx, gy = np.meshgrid((np.arange(42) - 20.5) * PITCH, (np.arange(32) - 15.5) * PITCH)
        sites = np.stack([gx.ravel(), gy.ravel()], -1)
        free = sites[(np.linalg.norm(sites[:, None] - fixed[None], axis=-1) > 0.06).all(axis=1)]
        free = free[np.argsort(np.linalg.norm(free, axis=-1), kind='stable')][:s.N - len(fixed)]
        assert len(free) == s.N - len(fixed)
        ids = (11 * np.arange(len(fixed)) + 5) % s.N          # (11 and 1024 are coprime: distinct ids)
        rest = np.setdiff1d(idx, ids)
        xy[:, ids] = fixed
        xy[:, rest] = free
    else:
        xy[:, :, 0] = (idx % side - (side - 1) / 2.0) * PITCH - (0.2 if s.N == 1024 else 0.0)
        xy[:, :, 1] = (idx // side - (side - 1) / 2.0) * PITCH
        cluster = hexagon(s.rings) * SPACING + np.array([0.80, 0.0] if s.N == 1024 else [0.55, 0.0])
        stride = 16 if s.N == 1024 else 5
        xy[:, stride * np.arange(len(cluster)) + 3] = cluster
    xy += rng.uniform(-0.0002, 0.0002, size=xy.shape)
    th = rng.uniform(-np.pi, np.pi, size=(E, s.N))
    return xy, th


def actions(s, k):
    """fresh U([0, 0.01] x [-pi/2, pi/2]) commands for substep k (the fused launch: k = SINGLE_SUBSTEPS)"""
    return scenes.random_actions(E, s.N, seed=700 + 20 * len(s.name) + k)


# ---- what a substep has, from the oracle's packed list and poses ---------------------------------------------------------
def lists(ws_key, ws_cnt):
    """(owner [n], key [n]) of one env's packed list: owners in ascending id, ws_cnt[a] entries each"""
    owner = np.repeat(np.arange(len(ws_cnt)), np.asarray(ws_cnt).astype(np.int64))
    return owner, np.asarray(ws_key)[:len(owner)].astype(np.int64)


def pairs(ws_key, ws_cnt):
    """{(owner, partner)} of the kilobot - kilobot contacts of one env"""
    owner, key = lists(ws_key, ws_cnt)
    return {(int(a), int(b)) for a, b in zip(owner, key) if b < WALL_KEY}


def wall_contacts(ws_key, ws_cnt):
    owner, key = lists(ws_key, ws_cnt)
    return {(int(a), int(b)) for a, b in zip(owner, key) if b >= WALL_KEY}


def largest_island(ws_key, ws_cnt):
    N = len(ws_cnt)
    parent = list(range(N))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b in pairs(ws_key, ws_cnt):
        parent[find(a)] = find(b)
    return int(np.bincount([find(a) for a in range(N)], minlength=N).max())


def fullest_cell(xy_m):
    """kilobots in the fullest broadphase cell of one env (poses in metres)"""
    c = np.floor((np.asarray(xy_m, np.float64) - [XMIN, YMIN]) / CELL).astype(np.int64)
    c = np.clip(c, 0, [GW - 1, GH - 1])
    return int(np.bincount(c[:, 1] * GW + c[:, 0]).max())


def substep_features(osim, before):
    """Per env a dict of what the substep that the oracle just made has; before: per env the (pairs, wall contacts) of the
    substep in front of it, or None.  The list the NEXT substep's lookups read is this substep's, the cells the label pass of
    this substep ranked are those of the poses it started from: both are taken after the substep, one substep apart at most,
    which is what the conditions of tests/test_label_pass_cpu.py are about (scenes that keep their features over substeps)."""
    out = []
    xy = osim.poses_m()[..., :2]
    for e in range(osim.ws_cnt.shape[0]):
        pr, wl = pairs(osim.ws_key[e], osim.ws_cnt[e]), wall_contacts(osim.ws_key[e], osim.ws_cnt[e])
        f = dict(contacts=int(osim.ws_cnt[e].astype(np.int64).sum()),
                 long_owners=int((osim.ws_cnt[e] > LONG_LIST).sum()), longest=int(osim.ws_cnt[e].max()),
                 fullest_cell=fullest_cell(xy[e]), island=largest_island(osim.ws_key[e], osim.ws_cnt[e]),
                 pairs=pr, walls=wl, owner_changes=0, walls_kept=0)
        if before is not None:
            f['owner_changes'] = sum(1 for a, b in pr if (b, a) in before[e][0])
            f['walls_kept'] = len(wl & before[e][1])
        out.append(f)
    return out
