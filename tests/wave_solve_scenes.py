"""Scenes for the stretch of the register solver that a wave runs through on its own (kb_regsolve_bins.inc: warm start, ten
velocity sweeps, StoreImpulses, integration, position sweeps -- no workgroup barrier in between).

Two things can go wrong there that no other phase can get wrong:

    order       a wave that is done with its velocity sweeps integrates and starts its position sweeps while other waves are
                still in their set-up or their velocity sweeps: whatever it writes early (positions, start-of-substep poses
                over arrays of the earlier phases, island flags) must be something no other wave reads
    ownership   a kilobot with a swept contact is integrated by the lane that holds its last contact in canonical order, every
                other one by its owner thread, which learns it from a marker bit written by the grouping pass: every kilobot
                must be integrated exactly once

What the scenes are made of (metres; kilobot diameter 33 mm, linear slop 0.2 mm, an island's position sweeps go on while a
contact is deeper than 3 slop = 0.6 mm):

    mesh        a hexagonal patch 32.8 mm apart, at rest: the largest island (it goes to wave 0), many depth levels, ONE
                position iteration
    deep ...    pairs, rows of three and a hexagon of seven that overlap by 1 .. 25 mm, at rest: the smallest islands (they go to
                the last waves), one or two depth levels, four to ten position iterations in the first launches
    shallow     pairs 32.8 mm apart, at rest: one iteration
    pair, row, hex6, hex12
                moving kilobots with 1, 2, 6 and 12 contacts (the second kilobot of a pair is only ever a contact's partner)
    walls       kilobots on the lower wall and one in the corner, moving
    sleepers    a block asleep from the start; dozer: a block at rest whose middle kilobot spins until launch DOZE, so that
                the block falls asleep inside the fused launch; leaver: a block asleep with a sleeping neighbour that is
                commanded away from launch LEAVE on (its command wakes it, and with it the block)
    ram         a kilobot that runs head-on into the left wall at full speed and meets it in launch 0: a candidate of the
                continuous step
    rafts       two patches side by side, both headed left: the right one is driven into the left one (one island, too large
                for a wave: the cooperative sweep), then the left one is driven away (two islands: the register path again)
    filler      single kilobots on a lattice, moving: no contact

Which wave holds an island and how many iterations its position sweeps take does not show in what the oracle returns; the
placement rule is the one restated in tests/setup_scenes.py (wave_loads), the iterations of a pair at rest follow from the
closed form below (pair_after).  Shared by tests/test_wave_solve_cpu.py and tests/test_wave_solve_gpu.py."""
import functools
from types import SimpleNamespace

import numpy as np

from tests import label_scenes as LS
from tests import scenes
from tests import setup_scenes as SS
from tests import toi_scenes as TS
from tests.scenes import case_id  # noqa: F401

f32 = np.float32
WORLD = 25.0
DIAMETER = 0.033
SLOP, BAUMGARTE = 0.005, 0.2            # world units (b2_linearSlop), b2_baumgarte
POS_ITERS = 10
SINGLE_LAUNCHES, FUSED_SUBSTEPS = 12, 10
SPEED = 0.25                            # of the commanded linear velocity of the moving kilobots
FULL = 0.01
PITCH = 0.045                           # of the filler lattice
DOZE, LEAVE = 9, 6                      # launch from which the dozer's middle rests / the leaver is commanded away
MERGE, PART = (1, 5), 6                 # launches in which the right raft is driven / from which the left one is
DEEP_MM = (32.1, 31.5, 29.0, 28.5, 24.0, 15.0, 8.0)      # centre distances of the deep pairs

_S = lambda name, N, envs, has, sleep_only=False: SimpleNamespace(name=name, N=N, envs=envs, has=has, sleep_only=sleep_only)      # noqa: E731
_DEEP = ['deep%g' % d for d in DEEP_MM]
SCENES = [
    # env 0: wave 0 deep in levels with one position iteration, the last waves shallow with many; env 1 the other way round
    _S('out-of-step-1024', 1024, [['mesh3'] + _DEEP * 5 + ['deeprow'] * 8 + ['ram'], ['deephex'] + ['shallow'] * 60], ('out of step', 'ram')),
    _S('everybody-1024', 1024, [['walls', 'hex12', 'hex6'] + ['row'] * 20 + ['pair'] * 40 + _DEEP, ['walls', 'hex12', 'hex6', 'hex6'] + ['row'] * 30 + ['pair'] * 20],
       ('everybody',)),
    _S('sleep-1024', 1024, [['sleepers', 'dozer', 'leaver', 'walls'] + ['pair'] * 40 + _DEEP, ['dozer', 'sleepers', 'leaver'] + ['row'] * 30 + ['deeprow'] * 4],
       ('sleep',), sleep_only=True),
    _S('rafts-1024', 1024, [['rafts'] + ['pair'] * 30, ['mesh3'] + ['pair'] * 40 + _DEEP], ('path change',)),
    # the generic kernel of two waves, and a one-wave workgroup
    _S('mixed-200', 200, [['mesh2', 'walls', 'hex6', 'ram'] + _DEEP + ['pair'] * 10 + ['row'] * 5, ['deephex', 'walls', 'hex6'] + ['shallow'] * 12 + ['pair'] * 10 + ['row'] * 4],
       ('out of step', 'everybody', 'ram')),
    _S('sleep-200', 200, [['sleepers', 'dozer', 'leaver', 'walls'] + ['pair'] * 10 + _DEEP, ['dozer', 'leaver'] + ['row'] * 10], ('sleep',), sleep_only=True),
    _S('mixed-64', 64, [['walls', 'hex6'] + _DEEP[:4] + ['pair'] * 4 + ['row'] * 3, ['deephex', 'walls', 'hex6'] + ['shallow'] * 4 + ['pair'] * 4 + ['row'] * 2], ('everybody',)),
    _S('sleep-64', 64, [['sleepers3', 'dozer', 'leaver'] + ['pair'] * 4, ['dozer', 'leaver', 'walls'] + ['row'] * 3], ('sleep',), sleep_only=True),
]


cases = functools.partial(scenes.sleep_cases, SCENES)      # (scene, allow_sleep) of both test files


# ---- structures: (xy [n, 2] metres around the lower left of the structure, role [n], heading or None) ------------------------
def _grid(nx, ny, d):
    i = np.arange(nx * ny)
    return np.stack([i % nx, i // nx], -1) * d


def structure(kind):
    if kind.startswith('mesh'):
        return LS.hexagon(int(kind[4:])) * 0.0328, 'rest', None
    if kind.startswith('deep') and kind[4:5].isdigit():
        return np.array([[0.0, 0.0], [float(kind[4:]) * 1e-3, 0.0]]), 'rest', None
    if kind == 'deeprow':
        return np.array([[0.0, 0.0], [0.0285, 0.0], [0.057, 0.0]]), 'rest', None
    if kind == 'deephex':
        return LS.hexagon(1) * 0.0285, 'rest', None
    if kind == 'shallow':
        return np.array([[0.0, 0.0], [0.0328, 0.0]]), 'rest', None
    if kind == 'pair':
        return np.array([[0.0, 0.0], [0.032, 0.0]]), 'move', None
    if kind == 'row':
        return np.array([[0.0, 0.0], [0.032, 0.0], [0.064, 0.0]]), 'move', None
    if kind == 'hex6':
        return LS.hexagon(1) * 0.032, 'move', None
    if kind == 'hex12':
        return LS.hexagon(2) * 0.019, 'move', None
    if kind in ('sleepers', 'sleepers3'):
        n = 3 if kind == 'sleepers3' else 4
        return _grid(n, n, 0.0325), 'asleep', None
    if kind == 'dozer':
        return _grid(3, 3, 0.0328), ['rest'] * 4 + ['spin'] + ['rest'] * 4, None
    if kind == 'leaver':
        return np.concatenate([_grid(3, 3, 0.0328), [[3 * 0.0328, 0.0328]]]), ['asleep'] * 9 + ['leave'], 0.0
    if kind == 'rafts':
        left = LS.hexagon(3) * 0.0328
        right = left + np.array([left[:, 0].max() - left[:, 0].min() + 0.0345, 0.0])
        return np.concatenate([left, right]), ['raftL'] * len(left) + ['raftR'] * len(left), np.pi
    raise KeyError(kind)


def walls_xy(N):
    """kilobots 1.5 mm inside the lower wall's skin (40 mm apart), the last one in the lower left corner"""
    n = 6 if N >= 200 else 4
    w = np.stack([-0.60 + 0.04 * np.arange(n), np.full(n, -0.75 + 0.015)], -1)
    w[-1] = (-1.0 + 0.015, -0.75 + 0.015)
    return w


def ram_pose():
    """(x, y, heading) in metres of the kilobot that meets the left wall in launch 0 (tests/toi_scenes.py: 'ram')"""
    total = float(TS.thresholds(TS.DEFAULT_RADIUS)[0])
    x, y, th = TS.at_wall(0, total + 0.004, 5.0)
    return x / WORLD, y / WORLD, th


def plant_env(N, kinds, rng):
    """(xy [N, 2] metres, theta [N], role [N] of str, {kind: [ids of each of its structures]})"""
    xlim, ylim = (0.92, 0.66) if N == 1024 else ((0.60, 0.40) if N == 200 else (0.40, 0.25))
    pts, role, theta, where = [], [], [], {}
    cur = [-xlim, -ylim + 0.08, 0.0]        # shelf: next x, its y, its height

    def add(kind, xy, r, th):
        where.setdefault(kind, []).append(np.arange(len(pts), len(pts) + len(xy)))
        pts.extend(map(tuple, xy))
        role.extend([r] * len(xy) if isinstance(r, str) else r)
        theta.extend([np.nan if th is None else th] * len(xy))
    for kind in kinds:
        if kind == 'walls':
            add(kind, walls_xy(N), 'move', None)
            continue
        if kind == 'ram':
            x, y, th = ram_pose()
            add(kind, [(x, y)], 'ram', th)
            continue
        xy, r, th = structure(kind)
        xy = xy - xy.min(0)
        w, h = xy.max(0)
        if cur[0] + w > xlim:
            cur[0], cur[1], cur[2] = -xlim, cur[1] + cur[2] + 0.075, 0.0
        assert cur[1] + h < ylim, 'the shelves are full: %s' % kind
        add(kind, xy + np.array([cur[0], cur[1]]), r, th)
        cur[0] += w + 0.075
        cur[2] = max(cur[2], h)
    planted = np.array(pts).reshape(-1, 2)
    need = N - len(pts)
    assert need >= 0, 'too many kilobots planted: %d of %d' % (len(pts), N)
    gx, gy = np.meshgrid(np.arange(-0.92, 0.93, PITCH), np.arange(0.68, -0.69, -PITCH))
    sites = np.stack([gx.ravel(), gy.ravel()], -1)
    if len(planted):
        sites = sites[(np.linalg.norm(sites[:, None] - planted[None], axis=-1) > 0.062).all(axis=1)]
    assert len(sites) >= need, 'no room for %d fillers (%d sites)' % (need, len(sites))
    add('filler', sites[:need], 'move', None)
    perm = rng.permutation(N)               # ids in no relation to places
    xy = np.zeros((N, 2))
    xy[perm] = np.array(pts)
    th = np.array(theta)
    th = np.where(np.isnan(th), rng.uniform(-np.pi, np.pi, size=N), th)
    out_th, out_role = np.zeros(N), np.empty(N, object)
    out_th[perm] = th
    out_role[perm] = np.array(role, object)
    return xy, out_th, out_role, {k: [perm[v] for v in vs] for k, vs in where.items()}


def plant(s):
    """(xy [E, N, 2] metres, theta [E, N], sleep_time [E, N] (-1: asleep), role [E, N], per env {kind: [ids]})"""
    rng = np.random.RandomState(6000 + s.N + 7 * len(s.name))
    E = len(s.envs)
    xy, th, role, ids = np.zeros((E, s.N, 2)), np.zeros((E, s.N)), np.empty((E, s.N), object), []
    for e, kinds in enumerate(s.envs):
        xy[e], th[e], role[e], where = plant_env(s.N, kinds, rng)
        ids.append(where)
    st = np.where((role == 'asleep') | (role == 'leave'), -1.0, 0.0).astype(np.float32)
    return xy, th, st, role, ids


def actions(s, k, role):
    """commands of launch k: the moving kilobots get fresh U([0, 0.01] x [-pi/2, pi/2]) with SPEED of the speed, and never
    less than a tenth of it: a skipped or doubled integration moves them by 0.6 um and more, where a float of the positions
    has steps of 0.08 um at most"""
    a = scenes.random_actions(len(s.envs), s.N, seed=1100 + 20 * len(s.name) + k)
    a[..., 0] = SPEED * np.maximum(a[..., 0], 0.1 * FULL)
    a[role != 'move'] = 0.0
    a[role == 'ram'] = (FULL, 0.0)
    if k < DOZE:
        a[role == 'spin'] = (0.0, 1.0)
    if k >= LEAVE:
        a[role == 'leave'] = (FULL, 0.0)
    if MERGE[0] <= k <= MERGE[1]:
        a[role == 'raftR'] = (FULL, 0.0)
    if k >= PART:
        a[role == 'raftL'] = (FULL, 0.0)
    return a.astype(np.float32)


# ---- the position sweeps of a pair at rest, closed form ------------------------------------------------------------------
def pair_iterations(sep):
    """iterations of the position sweeps of an island that is one kilobot pair of separation `sep` (world units, negative:
    overlap): an iteration that finds the pair deeper than 3 slop asks for another one, up to POS_ITERS"""
    n = 1
    while sep < -3.0 * SLOP and n < POS_ITERS:
        sep += -min(max(BAUMGARTE * (sep + SLOP), -0.2), 0.0)
        n += 1
    return n


def pair_after(dist, n):
    """centre distance (world units) of a pair at rest after n iterations: every iteration moves the two kilobots apart by
    -C = -clamp(baumgarte (sep + slop), -maxLinearCorrection, 0) together, so that sep + slop shrinks by the factor 0.8"""
    sep = dist - DIAMETER * WORLD
    for _ in range(n):
        sep += -min(max(BAUMGARTE * (sep + SLOP), -0.2), 0.0)
    return sep + DIAMETER * WORLD


def degrees(ws_key, ws_cnt):
    """(kilobot contacts [N], wall contacts [N], entries owned [N]) per kilobot of one env"""
    owner, key = LS.lists(ws_key, ws_cnt)
    N = len(ws_cnt)
    kk = key < LS.WALL_KEY
    deg = np.bincount(owner[kk], minlength=N) + np.bincount(key[kk], minlength=N)
    return deg, np.bincount(owner[~kk], minlength=N), np.asarray(ws_cnt).astype(np.int64)
