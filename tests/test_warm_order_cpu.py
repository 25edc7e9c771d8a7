"""The warm start of the register solver rides in the rounds of the depth pass (kb_regsolve_bins.inc): a contact's
`v -+ im * acc * n` is applied in the round that gives the contact its depth level, where Box2D's WarmStart goes through the
contacts in canonical key order.  Stated here without a GPU, on contact lists of the oracle: in float32, one rounded operation
after the other as the kernel is compiled (-ffp-contract=off),

    canonical   key by key ((class, rank bucket) ascending), rank by rank inside the open-ended bucket, the contacts of one
                round in list order
    by level    depth level by depth level, the contacts of one level in REVERSED list order

leave every body velocity equal bit for bit: two contacts of one round never share a body, a contact's impulse `acc * n`
depends on nothing another contact writes, and sweeping by level keeps the relative order of any two contacts that share a
body.  The contacts, their canonical order and their levels come from tools/placement_model.py (the depth pass restated); the
impulses are the oracle's own (ws_acc after the substep: what the next warm start applies), the body velocities arbitrary
float32 numbers.  Scenes: the hexagonal cluster of tests/setup_scenes.py (a body with twelve contacts, ranks in the open-ended
bucket) and its scene with kilobots on a wall and in a corner (two wall contacts on one body)."""
import os
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import setup_scenes as SS

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import placement_model as PM  # noqa: E402

f32 = np.float32
IM_BOT = f32(1.0) / f32(0.0034)           # any float32 does: the statement is about the order, not the mass
WALL_NORMALS = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)]       # kb_common.h: wall_geom


def env_records(osim, e, x0, y0):
    """[(class, rank, A, B, acc, nx, ny)] of env e in list order (A < 0: wall -1 - A), with the oracle's impulses and the
    normals of the poses the substep started from"""
    cnt = osim.ws_cnt[e]
    n = int(cnt.astype(np.int64).sum())
    owner = np.repeat(np.arange(len(cnt)), cnt.astype(np.int64))
    acc = {}
    for a, k, v in zip(owner, osim.ws_key[e][:n].astype(np.int64), osim.ws_acc[e][:n]):
        a, k = int(a), int(k)
        acc[(-1 - (k - PM.WALL_KEY), a) if k >= PM.WALL_KEY else (a, k)] = f32(v)
    out = []
    for cls, rank, a, b in PM.env_contacts(x0[e], y0[e], osim.ws_key[e], cnt):
        if a < 0:
            nx, ny = WALL_NORMALS[-1 - a]
        else:
            dx, dy = f32(x0[e, b] - x0[e, a]), f32(y0[e, b] - y0[e, a])
            ln = np.sqrt(f32(f32(dx * dx) + f32(dy * dy)))
            nx, ny = (f32(dx / ln), f32(dy / ln)) if ln > 0 else (1.0, 0.0)
        out.append((cls, rank, a, b, acc[(a, b)], f32(nx), f32(ny)))
    return out


def warm_start(vel, recs, order):
    """b2ContactSolver::WarmStart over `recs` in `order`, float32, every operation rounded on its own; a wall is a body at rest
    with inverse mass 0 whose velocity nobody reads"""
    v = vel.copy()
    for i in order:
        _, _, a, b, acc, nx, ny = recs[i]
        px, py = f32(acc * nx), f32(acc * ny)
        if a >= 0:
            v[a, 0] = f32(v[a, 0] - f32(IM_BOT * px))
            v[a, 1] = f32(v[a, 1] - f32(IM_BOT * py))
        v[b, 0] = f32(v[b, 0] + f32(IM_BOT * px))
        v[b, 1] = f32(v[b, 1] + f32(IM_BOT * py))
    return v


def canonical_order(recs):
    """key by key, rank by rank in the open-ended bucket, list order inside a round"""
    rnd = lambda r: (r[0], min(r[1], PM.RK - 1), max(r[1], PM.RK - 1))      # noqa: E731
    return sorted(range(len(recs)), key=lambda i: (rnd(recs[i]), i))


def level_order(recs, N):
    """depth level by depth level, the contacts of a level in reversed list order"""
    _, depth = PM.islands_and_depths([r[:4] for r in recs], N)
    return sorted(range(len(recs)), key=lambda i: (depth[i], -i)), depth


@pytest.mark.parametrize('name', ['cluster-1024', 'walls-1024'])
def test_warm_start_by_depth_level_equals_the_canonical_order(name):
    s = next(s_ for s_ in SS.SCENES if s_.name == name)
    E = len(s.envs)
    xy, th, st, ids = SS.plant(s)
    osim = O.OracleSim(O.default_config(E, s.N, allow_sleep=0))
    osim.set_poses_m(xy, th)
    seen_bucket = seen_deep = seen_corner = seen_impulse = False
    for k in range(2):
        x0, y0 = osim.x.copy(), osim.y.copy()
        osim.set_actions(SS.actions(s, k, np.zeros_like(st)))
        osim.step(1)
        assert int(osim.status.max()) == 0
        for e in range(E):
            recs = env_records(osim, e, x0, y0)
            assert len(recs) == int(osim.ws_cnt[e].astype(np.int64).sum()) > 0
            by_level, depth = level_order(recs, s.N)
            canon = canonical_order(recs)
            assert by_level != canon, 'the two orders must differ for the comparison to say anything'
            vel = np.random.RandomState(11 * k + e).uniform(-1, 1, size=(s.N, 2)).astype(f32)
            want, got = warm_start(vel, recs, canon), warm_start(vel, recs, by_level)
            assert np.array_equal(want.view(np.uint32), got.view(np.uint32)), (name, k, e)
            assert not np.array_equal(want.view(np.uint32), vel.view(np.uint32))
            seen_bucket |= any(r[1] >= PM.RK for r in recs)
            seen_deep |= max(depth) >= SS.DEEP
            walls = {}
            for r in recs:
                if r[2] < 0:
                    walls[r[3]] = walls.get(r[3], 0) + 1
            seen_corner |= any(n == 2 for n in walls.values())
            seen_impulse |= any(r[4] > 0 for r in recs)
    assert seen_impulse
    if name == 'cluster-1024':
        assert seen_bucket and seen_deep       # rounds rank by rank in the open-ended bucket; a body with twelve contacts
    else:
        assert seen_corner                     # two wall contacts on one body


def test_an_order_that_is_not_by_level_differs():
    """the comparison can fail: with the contacts of one body applied in another order the bits change"""
    s = next(s_ for s_ in SS.SCENES if s_.name == 'cluster-1024')
    xy, th, st, ids = SS.plant(s)
    osim = O.OracleSim(O.default_config(len(s.envs), s.N, allow_sleep=0))
    osim.set_poses_m(xy, th)
    x0, y0 = osim.x.copy(), osim.y.copy()
    osim.set_actions(SS.actions(s, 0, np.zeros_like(st)))
    osim.step(1)
    recs = env_records(osim, 0, x0, y0)
    vel = np.random.RandomState(3).uniform(-1, 1, size=(s.N, 2)).astype(f32)
    canon = canonical_order(recs)
    want, got = warm_start(vel, recs, canon), warm_start(vel, recs, canon[::-1])
    assert not np.array_equal(want.view(np.uint32), got.view(np.uint32))
