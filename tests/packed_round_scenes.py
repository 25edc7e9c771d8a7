"""Scenes for the rounds of the register solver that work on x/y pairs (kb_regsolve_bins.inc: the normal of the set-up, warm
start, velocity round, integration -- v_pk_mul_f32 / v_pk_add_f32 on aligned register pairs, kb_common.h: kb_pair; the position
round reads the same bodies component by component).  A packed lane can go wrong by a swapped or doubled component, a sign
applied to one half only, a broadcast that takes the wrong half, or a slot whose pair the allocator placed differently from the
other slot's.  None of that depends on the size of a scene, so the scenes are the smallest that have every kind of lane:

    slots-1024      the lattice of motifs of tests/setup_scenes.py ('dealt-1024'): by the placement rule (tools/placement_model.py)
                    an env has waves of more than 64 contacts -- both register slots, the warm-start pass level by level --
                    beside waves of at most 64 -- one slot, the warm start inside the depth rounds
    walls-1024      the same lattice with single kilobots driven into each of the four walls and into two corners (A is a wall:
                    inverse mass 0, normals (+-1, 0) and (0, +-1), two walls on one body) and one whose centre starts 2 mm
                    outside the left wall: its wall normal is flipped
    deep-1024       'cluster-1024': a hexagonal cluster whose middle kilobot touches twelve others, islands many levels deep
    rich-200        'mixed-200' of tests/setup_scenes.py, the generic sorted-bin kernel of two waves: cluster, walls, the pair
                    with coincident centres and the pair outside kb_exact_guard, <= 128 contacts per wave

Every 1024 scene runs with and without the sleep state and with the continuous step on and off (the four fixed-size
instantiations differ in the sleep state and sensing; sensing does not touch the solver), six single substeps and one fused
launch of ten.  The oracle runs once per case (reference()).  Shared by tests/test_packed_rounds_cpu.py (every scene has on
the oracle what it is there for) and tests/test_packed_rounds_gpu.py (every launch bit for bit)."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np

from oracle import oracle as O
from tests import setup_scenes as SS

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import placement_model as PM  # noqa: E402

SINGLE_LAUNCHES, FUSED_SUBSTEPS = 6, 10
FIELDS = ('x', 'y', 'theta', 'v', 'w', 'cmd_vx', 'cmd_vy', 'cmd_w', 'status')
WS = ('ws_cnt', 'ws_key', 'ws_acc')
MIN_DEPTH = 4
HX, HY = 1.0 - 0.97 * 0.0165, 0.75 - 0.97 * 0.0165      # centre 3 % of a radius inside the wall's skin (walls 0 .. 3: left, bottom, right, top)
# (x, y, heading, commanded speed): one kilobot per wall, two corners, and the one that starts outside the left wall
WALL_PLACES = [(-HX, 0.3, np.pi, 0.01), (0.2, -HY, -np.pi / 2, 0.01), (HX, -0.2, 0.0, 0.01), (-0.4, HY, np.pi / 2, 0.01),
               (-HX, HY, 3 * np.pi / 4, 0.01), (HX, -HY, -np.pi / 4, 0.01), (-1.002, -0.3, 0.0, 0.003)]
OUTSIDE = len(WALL_PLACES) - 1

_S = lambda name, src, has: SimpleNamespace(name=name, src=src, has=has)      # noqa: E731
SCENES = [_S('slots-1024', 'dealt-1024', ('slots',)), _S('walls-1024', 'dealt-1024', ('walls',)), _S('deep-1024', 'cluster-1024', ('deep',)),
          _S('rich-200', 'mixed-200', ('rich',))]
CASES = [(s.name, sleep, toi) for s in SCENES for sleep in (0, 1) for toi in (0, 1)]


def case_id(c):
    return '%s-sleep%d-toi%d' % c


def scene_of(name):
    return next(s for s in SCENES if s.name == name)


def fields_of(sleep):
    return FIELDS + (('sleep_time',) if sleep else ())


@functools.lru_cache(maxsize=None)
def start(name):
    """(N, xy [E, N, 2] metres, theta [E, N], launch k -> actions [E, N, 2], ids of the wall kilobots [E, 7] or None)"""
    s = scene_of(name)
    src = next(s_ for s_ in SS.SCENES if s_.name == s.src)
    xy, th, st, _ = SS.plant(src)
    awake = np.zeros_like(st)
    driven = None
    if 'walls' in s.has:
        driven = np.zeros((xy.shape[0], len(WALL_PLACES)), np.int64)
        for e in range(xy.shape[0]):
            d = np.linalg.norm(xy[e][:, None] - xy[e][None], axis=-1) + 10.0 * np.eye(src.N)
            singles = np.nonzero(d.min(1) > 0.04)[0]
            assert len(singles) >= len(WALL_PLACES)
            driven[e] = singles[:len(WALL_PLACES)]
            for i, (px, py, pth, _) in zip(driven[e], WALL_PLACES):
                xy[e, i], th[e, i] = (px, py), pth

    def actions(k):
        a = SS.actions(src, k, awake)
        if driven is not None:
            for e in range(a.shape[0]):
                a[e, driven[e]] = [(p[3], 0.0) for p in WALL_PLACES]
        return a.astype(np.float32)
    return src.N, xy, th, actions, driven


def launches():
    return [1] * SINGLE_LAUNCHES + [FUSED_SUBSTEPS]


def config_kw(sleep, toi):
    return dict(allow_sleep=sleep, toi_walls=toi)


def env_facts(x0, y0, ws_key, ws_cnt, nw):
    """What one substep of one env had, from the poses it started from and the packed list behind it: contacts per wave by
    the placement rule, the walls touched {kilobot: set of walls}, the deepest level of a contact"""
    N = len(ws_cnt)
    sizes = SS.islands(ws_key, ws_cnt)
    waves, rule = PM.place(sizes, nw)
    con = PM.env_contacts(x0, y0, ws_key, ws_cnt)
    _, depth = PM.islands_and_depths(con, N)
    return SimpleNamespace(ncon=sum(sizes), largest=sizes[0] if sizes else 0, rule=rule, loads=PM.loads(sizes, waves, nw),
                           walls={a: {int(k) - PM.WALL_KEY for k in ks} for a, ks in SS.wall_contacts_of(ws_key, ws_cnt).items()},
                           depth=max(depth, default=0))


@functools.lru_cache(maxsize=None)
def reference(case):
    """The oracle's state after every launch of the case, and what the single substeps had:
    [(fields + warm-start list as a namespace, [env_facts per env] or None for the fused launch, x, y in front of the launch)]"""
    name, sleep, toi = case
    N, xy, th, actions, _ = start(name)
    E = xy.shape[0]
    osim = O.OracleSim(O.default_config(E, N, O.DRIVE_VELOCITY, O.LIGHT_NONE, **config_kw(sleep, toi)))
    osim.set_poses_m(xy, th)
    nw = (8 if N == 1024 else 2)
    out = []
    for k, n in enumerate(launches()):
        x0, y0 = osim.x.copy(), osim.y.copy()
        osim.set_actions(actions(k))
        osim.step(n)
        snap = SimpleNamespace(cap=osim.cap, **{f: np.array(getattr(osim, f)) for f in fields_of(sleep) + WS})
        facts = [env_facts(x0[e], y0[e], snap.ws_key[e], snap.ws_cnt[e], nw) for e in range(E)] if n == 1 else None
        out.append((snap, facts, x0, y0))
    return out
