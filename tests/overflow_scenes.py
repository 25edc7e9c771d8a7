"""Scenes in which the warm-start store of kb_step overflows, in the two ways the status word names.

Status bit 1: a kilobot owns more contacts than kb_config.ws_slots (S).  The oracle defines what happens (oracle/kb_oracle.c,
`slot = nslot < S ? nslot : -1`): every contact is solved, the first S contacts of an owner in canonical order are stored
and warm-started, the others start from a zero impulse in every substep.  The device has code of its own for it in both
pipelines (kb_step_kernel.h: `mine > S`, M_XTRA / M_XFILL in the sorted-bin kernels, `slot >= S -> 255` in the linked-cell
kernels with objects or mixed laws).  SLOT_ROWS are the scenes that reach it.

Status bit 0: an env has more contacts than kb_config.contact_capacity.  Only the flag is specified for that env -- and that
the other envs of the launch are untouched.  CAPACITY_ROWS are launches of three envs whose MIDDLE env overflows: a list or
scratch record that leaves its slice lands in the slice of env 2 and shows as a mismatch there, not as an access beyond the
buffer.

Every scene has E = 3 envs, placed by scenes.lattice_spawn(3, N, seed=7, pitch, jitter=0.001) with single envs replaced by
scenes.gaussian_spawn(1, N, sigma, seed=21), and is driven by scenes.random_actions(3, N, seed=300 + launch).  (Two envs with
the Gaussian spawn start alike and part through their actions from the second substep on.)

Shared by tests/test_store_overflow_cpu.py (no row is vacuous on the oracle; which instantiation a row selects) and
tests/test_store_overflow_gpu.py (every launch of every row bit for bit against the oracle)."""
from types import SimpleNamespace

import numpy as np

from oracle import oracle as O
from tests import scenes

E = 3
LATTICE_SEED, GAUSS_SEED, JITTER = 7, 21, 0.001
ACTION_SEED = 300
TWIN_SLOTS = 64             # the twin of a slot row: the same scene with room for every contact (kb_create: ws_slots <= 64)
NCELL = 2494                # broadphase cells of the 2 x 1.5 m arena (tests/test_launch_cpu.py: ARENAS)
SPARSE_PITCH = 0.045        # a lattice without contacts
DENS = [2.0, 2.0, 1.0, 1.0, 1.0]        # KB_DRIVE_MIXED: the densities of the five laws (tests/test_mixed_laws.py)
BOX = (0.075, 0.05)         # half extents in metres of the 0.15 x 0.10 m box (tests/variant_census.py)

# a launch: (substeps, 'r' random actions | 'z' zero actions)
PLAIN = [(1, 'r')] * 6 + [(10, 'r')]
# the 0.034 m lattice stands apart at the start and closes up under the drive: a quarter of its kilobots own more than one
# contact from the twelfth substep on; up to the fourth the contacts fit the LDS staging area of the fixed-size kernel
CLOSING = [(1, 'r')] * 16 + [(10, 'r')]
# random actions, then rest for 7 launches of 10 substeps (the swarm falls asleep), then random actions again (the islands are
# woken through the truncated store)
SLEEPING = [(1, 'r')] * 3 + [(10, 'z')] * 7 + [(1, 'r')] * 4 + [(10, 'r')]

# The condition against vacuity of a slot row, in the twin with room for every contact:
#   QUARTER   in every flagged env at least a quarter of the kilobots own more than S contacts, in some single-substep launch
#   FEW       a square lattice on a pitch between the diameter / sqrt(2) and the diameter, S = 2: a kilobot inside the lattice
#             owns its east and its north neighbour and nothing else, so only kilobots that the jitter, the drive or an object
#             gave a third partner exceed two slots (2 .. 5 of 200 at the start) -- a quarter cannot.  What these rows hold
#             the device to is the other end of the overflow: a packed list with a handful of surplus contacts behind it.  At
#             least a quarter of the kilobots fill their S slots, and in every flagged env somebody exceeds them.
QUARTER, FEW = 'quarter', 'few'


def _row(kind, name, N, S, spawn, status, steps=PLAIN, over=QUARTER, flag_by=0, mode=O.DRIVE_VELOCITY, objects=0, shape=None,
         allow_sleep=0, capacity=0, solver_modes=(0,), threads=0):
    """spawn: per env ('lattice', pitch) or ('gauss', sigma).  status: what `status & 3` of every env is after every launch
    from launch `flag_by` on (before: no bit beyond it).  objects: bodies at the origin, shape None = the default disc or
    'box'.  solver_modes: kb_config.solver_mode values the device test runs the row under.  threads: what to ask of
    kb_set_block_threads (0: keep kb_create's width)."""
    return SimpleNamespace(kind=kind, name=name, N=N, S=S, spawn=spawn, status=tuple(status), steps=steps, over=over, flag_by=flag_by,
                           mode=mode, objects=objects, shape=shape, allow_sleep=allow_sleep, capacity=capacity, solver_modes=solver_modes,
                           threads=threads)


def _slot(name, N, S, spawn, status=(2, 2, 2), **kw):
    return _row('slot', '%s-n%d-s%d' % (name, N, S), N, S, spawn, status, **kw)


L31, L325, L34 = [('lattice', 0.031)] * 3, [('lattice', 0.0325)] * 3, [('lattice', 0.034)] * 3


def _dense(sigma):
    return [('gauss', sigma), ('gauss', sigma), ('lattice', SPARSE_PITCH)]


ALL_SOLVERS = (0, 1, 2, 3, 4)
# The straddle row exists for one condition: the stored entries fit the LDS staging area (capL = kb_lds_staging_entries, 280 at
# 200 kilobots) while the solved contacts do not, so that `big = newTotal + extras > capS` sends a substep to the global slice
# on the strength of the surplus alone.  With two slots a blob stores up to two entries per kilobot: on sigma = 0.05 m that is
# 340 .. 370, beyond capL.  On 0.13 m the rim of the blob is loose: 214 .. 272 stored, 298 .. 327 solved in every launch.
STRADDLE_SIGMA = 0.13
SLOT_ROWS = (
    [_slot('one-wave', 64, 1, L31)]
    + [_slot('one-wave-dense', 64, S, _dense(0.03), (2, 2, 0)) for S in (1, 2, 4, 8)]
    + [_slot('multi-wave', 200, 1, L31, solver_modes=ALL_SOLVERS), _slot('multi-wave', 200, 2, L31, over=FEW, solver_modes=ALL_SOLVERS)]
    + [_slot('straddle', 200, 2, _dense(STRADDLE_SIGMA), (2, 2, 0))]
    # (at two slots the first kilobots of the 0.0325 m lattice exceed them in the second to fourth substep)
    + [_slot('fixed-1024', 1024, 1, L325), _slot('fixed-1024', 1024, 2, L325, over=FEW, flag_by=3)]
    + [_slot('fixed-1024-lds', 1024, 1, L34, steps=CLOSING)]
    + [_slot('disc', N, 1, L31, objects=1) for N in (64, 200)]
    # (the disc at the origin gives the kilobots around it a third contact: 30 of 64, but 38 of 200)
    + [_slot('disc', 64, 2, L31, objects=1), _slot('disc', 200, 2, L31, objects=1, over=FEW)]
    + [_slot('sleep', N, 1, L31, steps=SLEEPING, allow_sleep=1) for N in (64, 200)]
    # (8 x 8 kilobots, two slots: in env 1 nobody has a third partner before the second substep)
    + [_slot('sleep', 64, 2, L31, steps=SLEEPING, allow_sleep=1, over=FEW, flag_by=1)]
    + [_slot('sleep', 200, 2, L31, steps=SLEEPING, allow_sleep=1, over=FEW)]
    # the other kernels: the kilobot - polygon kernels, both widths of the mixed-law kernel, the sleep twin of the
    # disc kernel; the last phase of SLEEPING wakes the islands
    + [_slot('box', N, 1, L31, objects=1, shape='box') for N in (64, 200)]
    + [_slot('mixed', N, 1, L31, mode=O.DRIVE_MIXED) for N in (64, 200)]
    + [_slot('disc-sleep', 64, 1, L31, objects=1, steps=SLEEPING, allow_sleep=1)]
    # the rows of 64 and 200 kilobots without objects all get the 80-VGPR budget (tier 2) from kb_create; the 128-VGPR
    # instantiation (tier 0) runs where the workgroup is narrowed by hand, as in tests/golden/variant_census.txt
    + [_slot('tier0', 128, 1, L31, threads=64), _slot('tier0-sleep', 128, 1, L31, threads=64, steps=SLEEPING, allow_sleep=1)]
)
SLEEP_ROWS = [r for r in SLOT_ROWS if r.allow_sleep]
STRADDLE = next(r for r in SLOT_ROWS if r.name.startswith('straddle'))
CONTACTS_SLOT_ROW = next(r for r in SLOT_ROWS if r.name == 'multi-wave-n200-s2')


def _cap(name, N, capacity, sigma, pitch, status, **kw):
    return _row('capacity', 'cap-' + name, N, 32, [('lattice', pitch), ('gauss', sigma), ('lattice', pitch)], status,
                steps=[(1, 'r')] * 3, capacity=capacity, **kw)


CAPACITY_ROWS = [
    _cap('small', 64, 160, 0.03, 0.031, (0, 1, 0)),
    _cap('small-sleep', 64, 160, 0.03, 0.031, (0, 1, 0), allow_sleep=1),
    _cap('default-200', 200, 0, 0.03, 0.031, (0, 3, 0)),
    _cap('default-256', 256, 0, 0.03, 0.031, (0, 3, 0)),
    _cap('fixed-1024', 1024, 0, 0.12, 0.0325, (0, 3, 0)),       # (4160, the only capacity the fixed-size kernel takes)
    _cap('disc', 64, 200, 0.03, 0.031, (0, 1, 0), objects=1),
]
MIDDLE, OUTER = 1, (0, 2)
OUTER_MIN_CONTACTS = 100
CONTACTS_CAPACITY_ROW = next(r for r in CAPACITY_ROWS if r.name == 'cap-default-200')
RECOVERY_SEED, RECOVERY_LAUNCHES = 9, 3      # after the overflow: scenes.lattice_spawn(3, N, seed=9, pitch=0.045), three launches


def row_id(r):
    return r.name


def config_kw(r, ws_slots=None, solver_mode=0):
    """Keywords of oracle.default_config / KilobotSim / tests.gpu_common.make_pair (drive mode and light go by position)."""
    kw = dict(ws_slots=r.S if ws_slots is None else ws_slots, allow_sleep=r.allow_sleep, contact_capacity=r.capacity, solver_mode=solver_mode)
    if r.mode == O.DRIVE_MIXED:
        kw.update(mode_density=DENS)
    if r.objects:
        kw.update(num_objects=r.objects)
        if r.shape == 'box':
            kw.update(obj_shape=[O.SHAPE_BOX] * r.objects, obj_nverts=[4] * r.objects,
                      obj_verts=[[[BOX[0] * O.WORLD_SCALE, BOX[1] * O.WORLD_SCALE]]] * r.objects)
    return kw


def plan_inputs(r):
    """The eleven inputs of plan_launch (columns of tests/golden/launch_plan.txt) of a row."""
    return [r.N, r.objects, r.objects, int(r.objects > 0 and r.shape is None), r.mode, O.LIGHT_NONE, 0, r.allow_sleep, NCELL, r.capacity, r.threads]


def start(r, order=None, seed_shift=0):
    """(xy [E, N, 2], th [E, N]) in metres / radians.  order: a permutation of the envs -- env i of the result is env order[i]
    of the row (tests/test_state_isolation_gpu.py puts the overflowing env first and last); None: the row's own order.
    seed_shift: added to both spawn seeds -- the twin scene of tests/guarded.py."""
    pitches = {p for kind, p in r.spawn if kind == 'lattice'}
    assert len(pitches) == 1
    xy, th = scenes.lattice_spawn(E, r.N, seed=LATTICE_SEED + seed_shift, pitch=pitches.pop(), jitter=JITTER)
    for e, (kind, sigma) in enumerate(r.spawn):
        if kind == 'gauss':
            gxy, gth = scenes.gaussian_spawn(1, r.N, sigma, seed=GAUSS_SEED + seed_shift)
            xy[e], th[e] = gxy[0], gth[0]
    if order is not None:
        assert sorted(order) == list(range(E))
        xy, th = xy[list(order)], th[list(order)]
    return xy, th


def object_start(r):
    """[E, M, 2] metres: the bodies rest at the origin, inside the swarm (None without objects)"""
    return np.zeros((E, r.objects, 2)) if r.objects else None


def state(r):
    """{buffer: array} written into both sims before the first launch: the laws and motors of a mixed swarm"""
    if r.mode != O.DRIVE_MIXED:
        return {}
    rng = np.random.RandomState(4000 + r.N)
    ml, mr = rng.randint(0, 256, (E, r.N)).astype(np.uint8), rng.randint(0, 256, (E, r.N)).astype(np.uint8)
    ml[rng.rand(E, r.N) < 0.3] = 0
    return dict(bot_mode=rng.randint(0, 5, (E, r.N)).astype(np.uint8), motor_l=ml, motor_r=mr)


def actions(r, k):
    a = scenes.random_actions(E, r.N, seed=ACTION_SEED + k)
    if r.steps[k][1] == 'z':
        a[...] = 0.0
    return a


def recovery_start(r):
    return scenes.lattice_spawn(E, r.N, seed=RECOVERY_SEED, pitch=SPARSE_PITCH)


def recovery_actions(r, k):
    return scenes.random_actions(E, r.N, seed=ACTION_SEED + len(r.steps) + k)


def fields(r):
    """What the device test compares bit for bit after every launch."""
    f = ('x', 'y', 'theta', 'v', 'w')
    if r.mode == O.DRIVE_MIXED:
        f += ('motor_l', 'motor_r')
    if r.objects:
        f += ('ox', 'oy', 'otheta', 'ovx', 'ovy', 'ow', 'ows_acc')
    if r.allow_sleep:
        f += ('sleep_time',) + (('osleep',) if r.objects else ())
    return f


def oracle_sim(r, ws_slots=None, solver_mode=0):
    o = O.OracleSim(O.default_config(E, r.N, r.mode, O.LIGHT_NONE, **config_kw(r, ws_slots, solver_mode)))
    o.set_poses_m(*start(r))
    if r.objects:
        o.set_objects_m(object_start(r))
    for name, val in state(r).items():
        getattr(o, name)[...] = val
    return o


def oracle_launch(o, r, k):
    o.set_actions(actions(r, k))
    o.step(r.steps[k][0])


def counts(ws_cnt):
    """stored entries per env from a [E, N] ws_cnt array"""
    return np.asarray(ws_cnt).astype(np.int64).sum(axis=1)


def owner_lists(ws_cnt, ws_key, ws_acc):
    """Per env and owner the stored list as (keys uint32, impulses as uint32 bit patterns) of one packed store."""
    ws_cnt = np.asarray(ws_cnt).astype(np.int64)
    key, acc = np.asarray(ws_key).view(np.uint32), np.ascontiguousarray(ws_acc, dtype=np.float32).view(np.uint32)
    out = []
    for e in range(ws_cnt.shape[0]):
        off = np.concatenate([[0], np.cumsum(ws_cnt[e])])
        out.append([(key[e, off[b]:off[b + 1]], acc[e, off[b]:off[b + 1]]) for b in range(ws_cnt.shape[1])])
    return out
