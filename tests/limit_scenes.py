"""Boundary scenes for the device-only staging limits (tests/limits_model.py): for every limit and every kernel class a pair
of scenes that differ by one kilobot,

    AT      the counted quantity equals the largest value that must still be bit-exact
    OVER    one more: the env is flagged, nothing else happens

each planted in env 0 of a three-env launch and again in the last env; the other envs hold an ordinary lattice (pitch 45 mm,
nobody touches).  Every scene is one substep: the piles burst in it.  Exact counts are found by search on the CPU, with the
model as the judge (tests/test_limits_cpu.py holds every row to its claim; tests/test_limits_gpu.py runs them on the device).

Kernel classes (what selects them is restated in `expected_shape` and checked against kb_create):

    hashed      sorted-bin kernel, cell heads in a hash table: N = 128 and 256 in the 2 x 1.5 m arena
    direct      sorted-bin kernel, one head per cell: N = 640 (a table of 2048 heads would not halve the 2494 cells)
    fixed1024   the fixed-size sorted-bin kernel (direct heads by construction)
    objects     N = 128 and one disc far away from everything: the one-wave kernel with objects
    mixed       KB_DRIVE_MIXED, N = 128: the one-wave mixed-law kernel
  solver_mode 0 stages the contacts in LDS as long as they fit kb_lds_staging_entries, solver_mode 3 always in the global slice:
  the two label passes of the sorted-bin kernels (:834 and :873).  The *-lds rows are sized so that their piles fit (the CPU
  test checks it); the piles of the partners rows never do -- 2080 contacts -- and take the second label pass under either mode.

Rows and the flag sites they sit on (kb_step_kernel.h unless named):

    rank-*          a (cell, direction) group of 256 contacts (largest rank 255) against 257: 16 kilobots just west of a cell
                    boundary, 16 just east of it, every pair across touches; OVER adds a kilobot in the western cell that
                    reaches exactly one of the eastern ones.  Label pass of the sorted-bin kernels (LDS staging / global staging)
                    and of the kernels with objects or mixed laws
    fixture-*       64 against 65 kilobots inside one disc or box (OBJ_LIST)
    depth-*         the deepest level of the cooperative sweep, 44 x waves - 2 against one more (kb_coopsolve_bins.inc): 86 / 87 at
                    the two waves of 128 kilobots, four neighbouring cells of 22 kilobots found by `search_depth`.  There is no
                    row at one wave (62 / 63 under kb_set_block_threads(64)): a one-wave workgroup never runs the level sweep
    candidates-*    candMax against candMax + 1 kilobots that run into the walls at full speed from just outside contact range
                    (status bit 3).  Where the perimeter has room they keep apart and touch nobody
    partners-*      64 partners of one kilobot in one direction.  OVER only: 63 partners cannot leave the status clean, the rank
                    limit of the partner cell's own group goes first (tests/limits_model.py says why), so these rows are flagged
                    by two sites at once -- the direction counters of the find pass and the label pass"""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import oracle as O
from tests import contact_search_scenes as CS
from tests import limits_model as LM
from tests import scenes
from tests import toi_scenes as TS

E = 3
CX, CY = 28, 21                              # the western cell of the piles; its eastern boundary and the middle of its row:
XB, Y0 = CS.XMIN + (CX + 1) * CS.CELL, CS.cell_centre(CX, CY)[1]
PITCH, JITTER, CLEAR = CS.PITCH, CS.JITTER, CS.CLEAR
FAR_DISC = np.array([-0.7, 0.5])             # the object of rows that only need the kernel with objects
SLOTS = 64                                   # ws_slots of every row: status bit 1 stays clear
WALL_PITCH, CROWDED_PITCH = 0.0332, 0.009    # along a wall: kilobots that must not touch (diameter 0.033), and kilobots that may
CORNER_MARGIN = 0.035                        # the walls are planted up to here from the corners: no two runners of different walls touch


# ---- planted kilobots ------------------------------------------------------------------------------------------------------
def rank_pile(n_west, n_east):
    west = [[XB - 0.001 - 0.0002 * i, Y0 + 0.003 * np.cos(i)] for i in range(n_west)]
    east = [[XB + 0.001 + 0.0002 * i, Y0 + 0.003 * np.sin(i)] for i in range(n_east)]
    return np.array(west + east)


def ring(n, radius=0.05):
    phi = 2 * np.pi * np.arange(n) / n
    return np.array([XB, Y0]) + radius * np.stack([np.cos(phi), np.sin(phi)], -1)


def wall_runners(n, pitch):
    """(xy [n, 2] metres, heading [n]): kilobots `pitch` apart along the four walls, 0.004 world units outside the contact
    radius and heading into the wall: at full speed they are inside b2TimeOfImpact's target distance after one substep.
    Walls in turn, from the middle of each wall outwards, clear of the corners."""
    total = float(TS.thresholds(TS.DEFAULT_RADIUS)[0])
    d = (total + 0.004) / TS.WORLD
    out = []
    per_wall = []
    for wl in range(4):
        half = (1.0 if wl in (1, 3) else 0.75) - CORNER_MARGIN
        k = int(half / pitch)
        per_wall.append([(wl, s * pitch) for s in sorted(range(-k, k + 1), key=abs)])
    i = 0
    while len(out) < n:
        wl = i % 4
        if per_wall[wl]:
            _, s = per_wall[wl].pop(0)
            x, y, th = TS.at_wall(wl, d * TS.WORLD, s * TS.WORLD)
            out.append((x / TS.WORLD, y / TS.WORLD, th))
        i += 1
        assert any(per_wall) or len(out) == n, 'the walls are full at this pitch'
    out = np.array(out)
    return out[:, :2], out[:, 2]


# ---- rows ------------------------------------------------------------------------------------------------------------------
def _row(name, limit, bit, N, kernel, mode=O.DRIVE_VELOCITY, solver_mode=0, objects=None, kw=None, block_threads=0, sites='',
         at_only=False, over_only=False):
    cfg = dict(allow_sleep=0, ws_slots=SLOTS, solver_mode=solver_mode)
    cfg.update(kw or {})
    if mode == O.DRIVE_MIXED:
        cfg.update(mode_density=[2.0, 2.0, 1.0, 1.0, 1.0])
    return SimpleNamespace(name=name, limit=limit, bit=bit, N=N, kernel=kernel, mode=mode, objects=objects, kw=cfg,
                           block_threads=block_threads, sites=sites, whiches=('at',) if at_only else ('over',) if over_only else ('at', 'over'))


DISC = dict(kw=dict(obj_radius=[0.075] * 8))
BOX = dict(kw=dict(obj_shape=[O.SHAPE_BOX] + [0] * 7, obj_nverts=[4] + [0] * 7,
                               obj_verts=[[[0.075 * 25.0, 0.075 * 25.0]] + [[0.0, 0.0]] * 3] + [[[0.0, 0.0]] * 4] * 7))

ROWS = [
    _row('rank-hashed-lds', 'rank', 4, 256, 'hashed', sites=':834', kw=dict(contact_capacity=4096)),      # (128 kilobots stage 352 contacts: the pile would go to the global slice)
    _row('rank-hashed-global', 'rank', 4, 128, 'hashed', solver_mode=3, sites=':873', kw=dict(contact_capacity=4096)),
    _row('rank-direct-lds', 'rank', 4, 640, 'direct', sites=':834', kw=dict(contact_capacity=4096)),
    _row('rank-direct-global', 'rank', 4, 640, 'direct', solver_mode=3, sites=':873', kw=dict(contact_capacity=4096)),
    _row('rank-fixed1024-lds', 'rank', 4, 1024, 'fixed1024', sites=':834'),
    _row('rank-fixed1024-global', 'rank', 4, 1024, 'fixed1024', solver_mode=3, sites=':873'),
    _row('rank-objects', 'rank', 4, 128, 'objects', objects='far', sites=':1158', kw=dict(contact_capacity=4096, **DISC['kw'])),
    _row('rank-mixed', 'rank', 4, 128, 'mixed', mode=O.DRIVE_MIXED, sites=':1158', kw=dict(contact_capacity=4096)),
    _row('fixture-disc', 'fixture', 4, 128, 'objects', objects='under', sites=':1015', kw=dict(contact_capacity=4096, **DISC['kw'])),
    _row('fixture-box', 'fixture', 4, 128, 'objects', objects='under', sites=':1015', kw=dict(contact_capacity=4096, **BOX['kw'])),
    _row('candidates-bins-256', 'candidates', 8, 256, 'hashed', sites=':2557', kw=dict(contact_capacity=200)),
    _row('candidates-objects-128', 'candidates', 8, 128, 'objects', objects='far', sites=':2557', kw=dict(contact_capacity=72, **DISC['kw'])),
    _row('candidates-mixed-128', 'candidates', 8, 128, 'mixed', mode=O.DRIVE_MIXED, sites=':2557', kw=dict(contact_capacity=88)),
    _row('candidates-fixed1024', 'candidates', 8, 1024, 'fixed1024', sites=':2557'),
    _row('partners-hashed-lds', 'partners', 4, 128, 'hashed', sites=':656 :873', kw=dict(contact_capacity=4096), over_only=True),
    _row('partners-hashed-global', 'partners', 4, 128, 'hashed', solver_mode=3, sites=':656 :873', kw=dict(contact_capacity=4096), over_only=True),
    _row('partners-fixed1024', 'partners', 4, 1024, 'fixed1024', sites=':656 :873', over_only=True),
    _row('partners-objects', 'partners', 4, 128, 'objects', objects='far', sites=':982 :1158', kw=dict(contact_capacity=4096, **DISC['kw']), over_only=True),
    _row('partners-mixed', 'partners', 4, 128, 'mixed', mode=O.DRIVE_MIXED, sites=':982 :1158', kw=dict(contact_capacity=4096), over_only=True),
    _row('depth-two-waves', 'depth', 4, 128, 'hashed', sites='kb_coopsolve_bins.inc:62', kw=dict(contact_capacity=4096)),
]
NON_INTERACTING = ('candidates-bins-256', 'candidates-objects-128', 'candidates-mixed-128')      # bit-3 rows whose kilobots touch nobody


def by_name(name):
    return next(r for r in ROWS if r.name == name)


def cases():
    return [(r, which, slot) for r in ROWS for which in r.whiches for slot in (0, E - 1)]


def case_id(c):
    return '%s-%s-env%d' % (c[0].name, c[1], c[2])


def expected_shape(row):
    """(hashed heads, fixed-size kernel, workgroup size) that the row's kernel class means, restating kb_launch.h: the heads
    are hashed where a power-of-two table of at least 2 N (and 64) entries is at most half the cells; N = 1024 is never"""
    H = 64
    while H < 2 * row.N:
        H <<= 1
    ncell = 58 * 43
    hashed = 2 * H <= ncell and row.N != 1024
    want = {'hashed': (True, False), 'direct': (False, False), 'fixed1024': (False, True),
            'objects': (hashed, False), 'mixed': (hashed, False)}[row.kernel]
    assert want[0] == hashed, row.name
    threads = row.block_threads or {'objects': 64, 'mixed': 64}.get(row.kernel, {128: 128, 256: 256, 640: 512, 1024: 512}[row.N])
    return want[0], want[1], threads


# ---- search ----------------------------------------------------------------------------------------------------------------
def fill(planted, N, rng):
    """[N, 2]: the planted kilobots, then the free lattice sites nearest to the middle of the arena"""
    gx, gy = np.meshgrid((np.arange(42) - 20.5) * PITCH, (np.arange(32) - 15.5) * PITCH)
    sites = np.stack([gx.ravel(), gy.ravel()], -1)
    if len(planted):
        sites = sites[(np.linalg.norm(sites[:, None] - planted[None], axis=-1) > CLEAR).all(axis=1)]
    need = N - len(planted)
    assert 0 <= need <= len(sites), (need, len(sites))
    sites = sites[np.argsort(np.linalg.norm(sites, axis=-1), kind='stable')][:need]
    return np.concatenate([planted.reshape(-1, 2), sites + rng.uniform(-JITTER, JITTER, size=sites.shape)])


def _objects(row, n_envs, planted_envs):
    if row.objects is None:
        return None
    objs = np.tile(FAR_DISC[None, None], (n_envs, 1, 1))
    if row.objects == 'under':
        for e in planted_envs:
            objs[e, 0] = [XB, Y0]
    return objs


def build(row, planted, heading=None, drive=None, slots=(0,), n_envs=1, seed=0):
    """A scene of n_envs envs with `planted` (metres) in the envs `slots`:
    SimpleNamespace(xy, th, actions, objects, state, ids [planted ids, the same in every planted env])"""
    rng = np.random.RandomState(4100 + row.N + seed)
    N, P = row.N, len(planted)
    xy, th = np.zeros((n_envs, N, 2)), rng.uniform(-np.pi, np.pi, size=(n_envs, N))
    act = scenes.random_actions(n_envs, N, seed=77 + seed)
    perm = np.random.RandomState(9 + row.N).permutation(N)       # ids in no relation to places, the same in every env
    for e in range(n_envs):
        mine = planted if e in slots else planted[:0]
        xy[e, perm] = fill(mine, N, np.random.RandomState(31 + e))
        if e in slots and heading is not None:
            th[e, perm[:P]] = heading
        if e in slots and drive is not None:
            act[e, perm[:P]] = drive
    state = {}
    if row.mode == O.DRIVE_MIXED:
        state['bot_mode'] = np.full((n_envs, N), O.DRIVE_VELOCITY, np.uint8)
    return SimpleNamespace(xy=xy, th=th, actions=act, objects=_objects(row, n_envs, slots), state=state, ids=perm[:P], row=row)


def oracle_sim(row, s, **changes):
    n_envs = s.xy.shape[0]
    kw = dict(row.kw)
    kw.update(changes)
    if s.objects is not None:
        kw['num_objects'] = s.objects.shape[1]
    osim = O.OracleSim(O.default_config(n_envs, row.N, row.mode, O.LIGHT_NONE, **kw))
    osim.set_poses_m(s.xy, s.th)
    if s.objects is not None:
        osim.set_objects_m(s.objects)
    for name, v in s.state.items():
        getattr(osim, name)[...] = v
    osim.set_actions(s.actions)
    return osim


def measure(row, planted, heading=None, drive=None):
    """the model's quantities of env 0 of the one-env scene with `planted`"""
    s = build(row, planted, heading, drive)
    return LM.evaluate(oracle_sim(row, s))[0]


def _quantity(row, q):
    return {'rank': q.max_rank, 'fixture': q.max_fixture, 'candidates': q.candidates, 'depth': q.depth, 'partners': q.max_partners}[row.limit]


@functools.lru_cache(None)
def planted(name, which, limit_value):
    """(xy [P, 2], heading or None, drive or None) of the row's AT / OVER scene.  limit_value: the largest exact value of
    the row's quantity (tests/limits_model.py: limits, of the row's handle); AT has exactly that, OVER one more."""
    row = by_name(name)
    want = limit_value + (which == 'over')
    if row.limit == 'rank':
        assert limit_value == 255
        pile = rank_pile(16, 16)
        if which == 'over':
            # one more kilobot in the western cell, on the row's middle line: moved in from out of reach until it touches
            # exactly one of the eastern kilobots
            for d in np.arange(0.0345, 0.0300, -0.00005):
                cand = np.concatenate([pile, [[XB - d, Y0]]])
                if measure(row, cand).max_rank >= want:
                    pile = cand
                    break
        got = (pile, None, None)
    elif row.limit == 'partners':
        # one kilobot just west of the boundary, `want` just east of it within reach
        east = [[XB + 0.001 + 0.00005 * i, Y0 + 0.004 * np.sin(i)] for i in range(want)]
        got = (np.array([[XB - 0.001, Y0]] + east), None, None)
    elif row.limit == 'fixture':
        got = (ring(want), None, None)
    elif row.limit == 'candidates':
        pitch = WALL_PITCH if name in NON_INTERACTING else CROWDED_PITCH
        xy, th = wall_runners(want, pitch)
        if name not in NON_INTERACTING:
            # kilobots that overlap along the wall push each other: plant one at a time until the model counts `want`
            n = want
            while True:
                xy, th = wall_runners(n, pitch)
                c = measure(row, xy, th, [TS.FULL, 0.0]).candidates
                if c >= want:
                    break
                assert c < want and n < row.N, (c, want, n)
                n += 1
        got = (xy, th, np.array([TS.FULL, 0.0], np.float32))
    elif row.limit == 'depth':
        got = depth_pile(name, want)
    else:
        raise KeyError(row.limit)
    q = measure(row, *got)
    assert _quantity(row, q) == want, '%s %s: the search ended at %s, wanted %d' % (name, which, _quantity(row, q), want)
    return got


# ---- depth: found by search over seed and pile size ----------------------------------------------------------------------
DEPTH_CELLS = ((CX, CY), (CX + 1, CY), (CX, CY + 1), (CX + 1, CY + 1))


def depth_candidate(seed, per_cell, spread):
    rng = np.random.RandomState(seed)
    return np.concatenate([CS.cell_centre(*c) + rng.uniform(-spread, spread, size=(per_cell, 2)) for c in DEPTH_CELLS])


def search_depth(name, limit, seeds=range(400)):
    """The search that filled DEPTH_FOUND (a fraction of a second on the oracle): four neighbouring cells with 18 .. 22 kilobots
    each within 4 .. 14 mm of the cell centres; a pile is taken if dropping kilobots from its end passes from limit + 1 levels
    to limit levels in one step, with every other quantity below its limit and more contacts than the register solver takes
    (the cooperative sweep must run: tests/solver_regimes.py).  -> [(seed, per cell, spread, dropped for limit + 1)]"""
    from tests import solver_regimes as SR
    row, found = by_name(name), []
    for seed in seeds:
        rng = np.random.RandomState(seed)
        per_cell, spread = int(rng.choice([18, 19, 20, 21, 22])), float(rng.choice([0.004, 0.006, 0.008, 0.010, 0.012, 0.014]))
        pile = depth_candidate(seed, per_cell, spread)
        if measure(row, pile).depth <= limit:
            continue
        qs = [measure(row, pile[:len(pile) - drop]) for drop in range(12)]
        for drop in range(11):
            pair = qs[drop], qs[drop + 1]
            if (pair[0].depth, pair[1].depth) == (limit + 1, limit) and all(
                    q.max_rank <= LM.RANK and q.max_partners <= LM.PARTNERS and q.ncon > SR.REG_CONTACTS * 2 for q in pair):
                found.append((seed, per_cell, spread, drop))
    return found


# (seed, kilobots per cell, spread in metres, kilobots dropped from the end): search_depth('depth-two-waves', 86, range(1))
DEPTH_FOUND = {('depth-two-waves', 87): (0, 22, 0.014, 0), ('depth-two-waves', 86): (0, 22, 0.014, 1)}


def depth_pile(name, want):
    seed, per_cell, spread, drop = DEPTH_FOUND[(name, want)]
    pile = depth_candidate(seed, per_cell, spread)
    return (pile[:len(pile) - drop], None, None)


@functools.lru_cache(None)
def row_limits(name):
    """(limits, shape) of the handle kb_create makes of the row's configuration (tests/limits_model.py: handle_limits)"""
    from gym_kilobots_amd import _native as nat
    from gym_kilobots_amd import build as kb_build
    kb_build.build()
    row = by_name(name)
    kw = dict(row.kw)
    if row.objects is not None:
        kw['num_objects'] = 1
    return LM.handle_limits(nat.load(), nat, kw, row.N, row.mode, block_threads=row.block_threads)


def scene(row, which, slot):
    """the three-env launch of a case"""
    xy, heading, drive = planted(row.name, which, getattr(row_limits(row.name)[0], row.limit))
    return build(row, xy, heading, drive, slots=(slot,), n_envs=E)
