"""The one-slot register set-up with the warm start in its depth rounds (kb_regsolve_bins.inc) on the device against the oracle,
bit for bit after every launch: poses, v, w, the sleep times where they are carried, the packed warm-start list (ws_cnt, ws_key,
ws_acc), status 0.

A wave of at most 64 contacts loads slot 0 once, leaves slot 1 idle and warm-starts inside the depth rounds; a wave of more
keeps the two-slot set-up and the warm-start pass by level.  Which of the two a wave takes shows in nothing the kernel returns,
so every row is classified from the DEVICE's own packed list and poses through the Python statement of the placement rule
(tools/placement_model.py) -- a row cannot silently stop visiting its case:

    one slot        every wave in use holds at most 64 contacts
    two slot        at least one wave of more than 64 contacts beside one-slot waves
    even            an island of 32 contacts or more: the env takes the even split
    rank bucket     contacts of rank RK - 1 and above (rounds rank by rank), in the crowded cells of the r = 0.008 m geometry
    walls           kilobots on one wall and one in a corner on two, with impulses from the launch before
    sleepers        (sleep instantiation) a sleeping island on a wave that also holds awake contacts: key 63 beside live rounds
    iterations      vel_iters = 0 (warm start, then integration only) and pos_iters = 0
    forget / fresh  the first launch after forget_contacts() (all impulses 0), and a fresh handle that continues from the
                    stored impulses
    fused           one launch of ten substeps against ten single launches

1024 kilobots run the fixed-size kernel of eight waves, 200 and 256 the generic kernel of two and four.  Every env of every
row must be on the register path (no island above GIANT_ISLAND, no wave above 128 contacts by the rule)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import scenes
from tests import setup_scenes as SS
from tests import solver_regimes as SR
from tests import placement_scenes as TP
from tests.gpu_common import make_pair, assert_same, assert_ws_same, cpu, dev

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import placement_model as PM  # noqa: E402

pytestmark = pytest.mark.gpu

LAUNCHES = 4
FIELDS = ('x', 'y', 'theta', 'v', 'w')
SLEEP_ISLAND = 24               # contacts of the 4 x 4 block of sleepers (tests/setup_scenes.py)

CROWD_R, CROWD_PITCH, CROWD_BLOCKS = 0.008, 0.0155, 20       # kilobots of 8 mm radius in 3 x 2 blocks, 0.5 mm of overlap
WALL_PLACES = 6                 # four kilobots driven into one wall each, two into corners

_R = lambda name, src, sleep, has, **kw: SimpleNamespace(name=name, src=src, sleep=sleep, has=has, kw=kw)      # noqa: E731
ROWS = [
    _R('one-slot-1024', ('setup', 'single-slot-1024'), 0, ('one slot',)),
    _R('two-slot-1024', ('setup', 'dealt-1024'), 0, ('two slot',)),
    _R('even-1024', ('setup', 'wave-counts-1024'), 0, ('even',)),
    _R('walls-1024', ('setup', 'walls-1024'), 0, ('two slot',)),
    _R('sleepers-1024', ('setup', 'sleepers-1024'), 1, ('sleepers',)),
    _R('sleepers-200', ('setup', 'sleepers-200'), 1, ('sleepers',)),
    _R('mixed-200', ('setup', 'mixed-200'), 0, ('even', 'rank bucket')),
    _R('crowded-200', ('crowded', None), 0, ('rank bucket', 'two slot')),
    _R('walls-256', ('walls', 'one-slot-256'), 0, ('one slot', 'walls')),
    _R('mix-256', ('placement', 'mix-256'), 0, ('two slot',)),
    _R('mix-256-vel0', ('placement', 'mix-256'), 0, ('two slot',), vel_iters=0),
    _R('mix-256-pos0', ('placement', 'mix-256'), 0, ('two slot',), pos_iters=0),
    _R('walls-256-pos0', ('walls', 'one-slot-256'), 0, ('one slot', 'walls'), pos_iters=0),
]


def crowded_scene(N=200, E=2):
    """r = 0.008 m: 3 x 2 blocks of kilobots, each inside one broadphase cell (35 mm) -- six kilobots and seven contacts in
    one (cell, direction) group, ranks 0 .. 6, so the open-ended bucket runs rank by rank -- and single kilobots between them.
    Twenty islands of seven contacts: by the packed rule nine of them fill the first wave's slot and the second wave takes
    the other eleven in two slots."""
    rng = np.random.RandomState(31)
    xy = np.zeros((E, N, 2))
    for e in range(E):
        pts = []
        for k in range(CROWD_BLOCKS):
            cx, cy = 6 + 4 * (k % 10), 8 + 6 * (k // 10)                # cell of the block
            x0, y0 = PM.XMIN / SS.WORLD + PM.CELL / SS.WORLD * cx + 0.002, PM.YMIN / SS.WORLD + PM.CELL / SS.WORLD * cy + 0.008
            pts += [(x0 + CROWD_PITCH * i, y0 + CROWD_PITCH * j) for j in range(2) for i in range(3)]
        pts += [(-0.9 + 0.05 * (k % 36), 0.2 + 0.05 * (k // 36)) for k in range(N - len(pts))]
        xy[e, rng.permutation(N)] = np.array(pts)
    xy += rng.uniform(-0.0001, 0.0001, size=xy.shape)
    return xy, rng.uniform(-np.pi, np.pi, size=(E, N))


def walls_scene(name):
    """A scene of tests/test_placement_gpu.py with six of its single kilobots moved: four against one wall each, two into
    corners, 3 % of a radius inside the wall's skin and heading into it; `driven` [E, 6] are their ids -- they get the full
    forward speed in every launch, so from the second launch on their wall contacts carry impulses."""
    s = next(s_ for s_ in TP.SCENES if s_.name == name)
    xy, th = TP.plant(s, seed=77 + s.N)
    hx, hy = 1.0 - 0.97 * 0.0165, 0.75 - 0.97 * 0.0165
    places = [(-hx, 0.3, np.pi), (0.2, -hy, -np.pi / 2), (hx, -0.2, 0.0), (-0.4, hy, np.pi / 2), (-hx, -hy, -3 * np.pi / 4), (hx, hy, np.pi / 4)]
    assert len(places) == WALL_PLACES
    driven = np.zeros((xy.shape[0], WALL_PLACES), np.int64)
    for e in range(xy.shape[0]):
        d = np.linalg.norm(xy[e][:, None] - xy[e][None], axis=-1) + 10.0 * np.eye(s.N)
        singles = np.nonzero(d.min(1) > 0.04)[0]
        assert len(singles) >= WALL_PLACES
        driven[e] = singles[:WALL_PLACES]
        for i, (px, py, pth) in zip(driven[e], places):
            xy[e, i], th[e, i] = (px, py), pth

    def actions(k):
        a = TP.actions(s, k)
        for e in range(a.shape[0]):
            a[e, driven[e]] = (0.01, 0.0)
        return a
    return s.N, xy, th, actions


def scene(row):
    """(N, xy [E, N, 2] metres, theta, sleep_time or None, actions(k), config keywords)"""
    kind, name = row.src
    kw = dict(row.kw)
    if kind == 'setup':
        s = next(s_ for s_ in SS.SCENES if s_.name == name)
        xy, th, st, _ = SS.plant(s)
        st = st if row.sleep else np.zeros_like(st)
        return s.N, xy, th, st if row.sleep else None, lambda k: SS.actions(s, k, st), kw
    if kind == 'crowded':
        xy, th = crowded_scene()
        kw.update(bot_radius=CROWD_R)

        def slow(k):
            a = scenes.random_actions(xy.shape[0], xy.shape[1], seed=50 + k)
            a[..., 0] *= SS.SPEED
            return a
        return xy.shape[1], xy, th, None, slow, kw
    if kind == 'walls':
        N, xy, th, actions = walls_scene(name)
        return N, xy, th, None, actions, kw
    s = next(s_ for s_ in TP.SCENES if s_.name == name)
    xy, th = TP.plant(s, seed=77 + s.N)
    return s.N, xy, th, None, lambda k: TP.actions(s, k), kw


def launch_facts(x0, y0, sleep0, prev_key, prev_acc, prev_cnt, ws_key, ws_cnt, nw):
    """What one launch had, per env, from the state in front of it and the packed list behind it (all from one backend)."""
    out = []
    for e in range(ws_cnt.shape[0]):
        N = ws_cnt.shape[1]
        sizes = SS.islands(ws_key[e], ws_cnt[e])
        waves, rule = PM.place(sizes, nw)
        load = PM.loads(sizes, waves, nw)
        f = SimpleNamespace(ncon=sum(sizes), sizes=sizes, rule=rule, loads=load,
                            one=sum(1 for c in load if 0 < c <= PM.SLOT), two=sum(1 for c in load if c > PM.SLOT))
        f.reg = bool(sizes) and sizes[0] <= SS.GIANT_ISLAND and max(load) <= PM.WAVE and sum(1 for n in sizes if n >= PM.CLASSES) <= 1
        con = PM.env_contacts(x0[e], y0[e], ws_key[e], ws_cnt[e])
        f.max_rank = max((c[1] for c in con), default=0)
        # wall contacts that were in the list of the launch before with an impulse: {kilobot: how many}
        owner = np.repeat(np.arange(N), prev_cnt[e].astype(np.int64))
        n0 = len(owner)
        had = {(int(a), int(k)) for a, k, v in zip(owner, prev_key[e][:n0], prev_acc[e][:n0]) if k >= PM.WALL_KEY and v > 0}
        f.warm_walls = {}
        owner = np.repeat(np.arange(N), ws_cnt[e].astype(np.int64))
        for a, k in zip(owner, ws_key[e][:len(owner)]):
            if (int(a), int(k)) in had:
                f.warm_walls[int(a)] = f.warm_walls.get(int(a), 0) + 1
        # the sleeping island: the only one of its size, so the rule fixes its wave; does that wave hold more than it?
        f.sleeper_shares = False
        if sleep0 is not None:
            lo, hi = con_of_sleepers(con, sleep0[e])
            if lo == SLEEP_ISLAND and hi == SLEEP_ISLAND and sizes.count(SLEEP_ISLAND) == 1 and f.reg:
                before = sum(n for n in sizes if n > SLEEP_ISLAND)          # contacts in front of it in walk order
                if rule == 'packed':
                    starts, counts, _ = PM.wave_starts(sizes, nw)
                    w = PM.wave_from_starts(starts, before)
                    f.sleeper_shares = counts[w] > SLEEP_ISLAND
                else:
                    chunk = max((f.ncon + nw - 1) // nw, 1)
                    f.sleeper_shares = load[min(before // chunk, nw - 1)] > SLEEP_ISLAND
        out.append(f)
    return out


def con_of_sleepers(con, sleep_time):
    """(contacts between two sleeping kilobots, contacts with at least one sleeping kilobot)"""
    both = sum(1 for _, _, a, b in con if a >= 0 and sleep_time[a] < 0 and sleep_time[b] < 0)
    any_ = sum(1 for _, _, a, b in con if (a >= 0 and sleep_time[a] < 0) or sleep_time[b] < 0)
    return both, any_


def check_row(row, seen, what):
    """seen: the facts of every env of every launch"""
    for f in seen:
        assert f.reg, '%s: not on the register path: %d contacts, islands %s, waves %s' % (what, f.ncon, f.sizes[:4], f.loads)
    if 'one slot' in row.has:
        assert all(f.two == 0 and f.one >= 2 and f.rule == 'packed' for f in seen), [(f.rule, f.loads) for f in seen]
    if 'two slot' in row.has:
        assert any(f.two >= 1 and f.one >= 1 and f.rule == 'packed' for f in seen), [(f.rule, f.loads) for f in seen]
    if 'even' in row.has:
        assert any(f.rule == 'even' and f.sizes[0] >= PM.CLASSES for f in seen), [(f.rule, f.sizes[:2]) for f in seen]
    if 'rank bucket' in row.has:
        assert any(f.max_rank >= PM.RK - 1 for f in seen) and any(f.max_rank >= PM.RK for f in seen), [f.max_rank for f in seen]
    if 'walls' in row.has:
        assert any(1 in f.warm_walls.values() for f in seen), 'no kilobot on one wall with an impulse from the launch before'
        assert any(2 in f.warm_walls.values() for f in seen), 'no kilobot in a corner with impulses from the launch before'
    if 'sleepers' in row.has:
        assert any(f.sleeper_shares for f in seen), 'no sleeping island on a wave with awake contacts'


def snapshot(gsim, sleep):
    return (cpu(gsim.x).copy(), cpu(gsim.y).copy(), cpu(gsim.sleep_time).copy() if sleep else None,
            cpu(gsim.ws_key).view(np.uint32).copy(), cpu(gsim.ws_acc).copy(), cpu(gsim.ws_cnt).copy())


def start_pair(row):
    N, xy, th, st, actions, kw = scene(row)
    osim, gsim = make_pair(xy.shape[0], N, xy=xy, th=th, allow_sleep=row.sleep, solver_mode=0, **kw)
    if row.sleep:
        osim.sleep_time[...] = st
        gsim.sleep_time.copy_(dev(st))
    assert xy.shape[0] <= 8 and gsim.block_threads // SR.LANES == {1024: 8, 256: 4, 200: 2}[N]
    return osim, gsim, actions, FIELDS + (('sleep_time',) if row.sleep else ())


def launch(osim, gsim, a, n, what, fields):
    osim.set_actions(a)
    osim.step(n)
    gsim.step(n, actions=dev(a))
    assert_same(osim, gsim, what, fields)
    assert_ws_same(osim, gsim, what)
    assert int(osim.status.max()) == 0 and int(cpu(gsim.status).max()) == 0, what


@pytest.mark.parametrize('row', ROWS, ids=lambda r: r.name)
def test_row_is_bit_exact_and_visits_its_case(row):
    osim, gsim, actions, fields = start_pair(row)
    nw = gsim.block_threads // SR.LANES
    seen = []
    for k in range(LAUNCHES):
        x0, y0, sl0, key0, acc0, cnt0 = snapshot(gsim, row.sleep)
        what = '%s launch %d' % (row.name, k)
        launch(osim, gsim, actions(k), 1, what, fields)
        facts = launch_facts(x0, y0, sl0, key0, acc0, cnt0, cpu(gsim.ws_key).view(np.uint32), cpu(gsim.ws_cnt), nw)
        print(what, [(f.ncon, f.rule, f.loads, f.max_rank, sorted(f.warm_walls.values()), f.sleeper_shares) for f in facts])
        seen += facts
    check_row(row, seen, row.name)


@pytest.mark.parametrize('name', ['mix-256', 'one-slot-1024'])
def test_forgotten_impulses_and_a_fresh_handle(name):
    """Two launches, forget_contacts() on both sides (every contact starts from impulse 0 as at the very first launch), two
    more launches, then a new handle takes over state and stored impulses and goes on."""
    from gym_kilobots_amd.sim import KilobotSim
    row = next(r for r in ROWS if r.name == name)
    osim, gsim, actions, fields = start_pair(row)
    for k in range(4):
        if k == 2:
            assert int(cpu(gsim.ws_cnt).astype(np.int64).sum()) > 0 and float(cpu(gsim.ws_acc).max()) > 0
            gsim.forget_contacts()
            osim.ws_cnt[...] = 0
        launch(osim, gsim, actions(k), 1, '%s launch %d' % (name, k), fields)
    torch.cuda.synchronize()
    assert float(osim.ws_acc[0, :int(osim.ws_cnt[0].astype(np.int64).sum())].max()) > 0     # impulses to continue from
    fresh = KilobotSim(gsim.x.shape[0], gsim.x.shape[1], O.DRIVE_VELOCITY, O.LIGHT_NONE, debug_outputs=True, allow_sleep=0, solver_mode=0)
    for f in FIELDS + ('ws_key', 'ws_acc', 'ws_cnt'):
        getattr(fresh, f).copy_(getattr(gsim, f))
    for k in range(4, 6):
        launch(osim, fresh, actions(k % LAUNCHES), 1, '%s fresh handle, launch %d' % (name, k), fields)


@pytest.mark.parametrize('name', ['two-slot-1024', 'sleepers-200'])
def test_one_fused_launch_equals_ten_single_launches(name):
    row = next(r for r in ROWS if r.name == name)
    osim, fused, actions, fields = start_pair(row)
    _, single, _, _ = start_pair(row)
    launch(osim, fused, actions(0), 1, name + ' first launch', fields)      # (stored impulses in front of the fused launch)
    single.step(1, actions=dev(actions(0)))
    a = actions(1)
    launch(osim, fused, a, SR.FUSED_SUBSTEPS, name + ' fused', fields)
    for _ in range(SR.FUSED_SUBSTEPS):
        single.step(1, actions=dev(a))
    assert_same(osim, single, name + ' ten single launches', fields)
    assert_ws_same(osim, single, name + ' ten single launches')
    assert int(cpu(single.status).max()) == 0


@pytest.mark.parametrize('name', ['walls-256', 'mix-256'])
def test_without_velocity_iterations_the_stored_impulses_are_warm_started(name):
    """vel_iters = 0 on its own never builds an impulse up.  So a pair with the default iterations runs two launches, and a
    pair with vel_iters = 0 takes over its state and its stored impulses: its substep is warm start, integration and position
    sweeps, and StoreImpulses hands the impulses on as they came."""
    row = next(r for r in ROWS if r.name == name)
    osim, gsim, actions, fields = start_pair(row)
    for k in range(2):
        launch(osim, gsim, actions(k), 1, '%s launch %d' % (name, k), fields)
    torch.cuda.synchronize()
    n = int(osim.ws_cnt[0].astype(np.int64).sum())
    assert float(osim.ws_acc[0, :n].max()) > 0
    o0, g0, _, _ = start_pair(SimpleNamespace(name=row.name, src=row.src, sleep=0, has=row.has, kw=dict(vel_iters=0)))
    for f in FIELDS + ('ws_key', 'ws_acc', 'ws_cnt'):
        getattr(o0, f)[...] = getattr(osim, f)
        getattr(g0, f).copy_(getattr(gsim, f))
    before = osim.ws_acc[0, :n].copy()
    for k in range(2, 4):
        launch(o0, g0, actions(k), 1, '%s vel_iters 0, launch %d' % (name, k), fields)
        if k == 2 and int(o0.ws_cnt[0].astype(np.int64).sum()) == n:
            assert np.array_equal(np.sort(o0.ws_acc[0, :n]), np.sort(before))
