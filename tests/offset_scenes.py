"""Every kernel where byte offsets pass 2^31 and 2^32: the batch sizes, the probe envs, the scenes and the table of the
entries.  Needs neither torch nor a device to import; what touches the device imports torch when it is called.

No other test puts an address more than a few hundred MiB behind the base of a tensor.  Here D = 5 distinct envs are tiled
to E envs -- env e carries scene e % D, every per-env input is a function of e % D --, E being the smallest multiple of D
that leaves at least D whole envs above the boundary a row claims.  The distinct envs are held to the restatement or to
the oracle, every replica to its distinct env, and the probe envs (the one that holds the first byte with bit 31 set, the
one with bit 32, the first env wholly above 2^32 and the last) once more to the restatement directly.  The env that
straddles the claimed boundary is no multiple of D, so that a byte offset that wraps to the front of the tensor puts
another scene's bits onto env 0's row.  Element indices stay below 2^31 in every row: byte offsets are the class under test.

Shared by tests/test_large_offsets_cpu.py (every size from the ABI constants, the scenes on the oracle, the table against
KilobotSim, the host refusals) and tests/test_large_offsets_gpu.py."""
import collections
import functools
from types import SimpleNamespace

import numpy as np

from oracle import oracle as O
from tests import residency_scenes as RS
from tests import scenes
from tests import solver_regimes as SR

D = RS.D
B31, B32 = 1 << 31, 1 << 32
FRONT_BAND = B31            # bytes of sentinel in front of every view under test: where a sign-extended 32-bit offset lands
SENTINEL = 0x5A             # every byte of a prefilled output: the word 0x5A5A5A5A is 1.5e9 as an int32 (no index, count or
SENTINEL_WORD = 0x5A5A5A5A  # code reaches it) and 1.5e16 as a float32 (no length, impulse or sum does)
HEADROOM = 1.25             # a GPU test runs if free memory >= need * HEADROOM

MAX_BOTS = 1024
MAX_CAPACITY = 65528                # kb_create: contact_capacity <= 65528
SCRATCH_BYTES_PER_CONTACT = 32      # kb_scratch_bytes = num_envs * capacity * 32
FIXED_1024_CAPACITY = 4 * MAX_BOTS + 64         # kb_launch.h: the capacity of the fixed-size kernel, a compile-time constant
HIST_MAX_BINS, MAX_NEIGHBORS, MAX_RAYS, GRID_MAX_SIDE, FIELD_MAX_CHANNELS, RENDER_MAX_SIDE = 64, 16, 32, 128, 4, 2048
REDUCE_MAX_CHANNELS, MAX_OBJECTS = 8, 8


# ---- the batch ------------------------------------------------------------------------------------------------------------
def straddler(row_bytes, boundary):
    """The env that holds byte `boundary` of a tensor of row_bytes per env: the first byte whose offset has that bit set."""
    return boundary // row_bytes


def first_above(row_bytes, boundary):
    """The first env that lies wholly at or above the boundary."""
    return -(-boundary // row_bytes)


def batch_envs(row_bytes, boundary):
    """The smallest multiple of D with at least D whole envs above the boundary."""
    return D * -(-(first_above(row_bytes, boundary) + D) // D)


def probes(row_bytes, E):
    """The envs that are pulled to the host, ascending: per boundary the tensor reaches its straddler and the first env
    wholly above it, and the last env."""
    out = {E - 1}
    for boundary in (B31, B32):
        if E * row_bytes > boundary:
            out |= {straddler(row_bytes, boundary), first_above(row_bytes, boundary)}
    return sorted(e for e in out if e < E)


def reached(row_bytes, E):
    """The highest of the two boundaries that a tensor of E rows passes, None if neither."""
    return B32 if E * row_bytes > B32 else B31 if E * row_bytes > B31 else None


# ---- row 1 and 2: the step kernels ----------------------------------------------------------------------------------------
# name; scene: how the D distinct envs start and what drives them; config keywords; the tensor whose rows claim the boundary
# and the bytes of one env's row of it; the boundary; masked: the masked step and reset follow; banded: the tensors that are
# moved behind a front band
def _regime_scene(name):
    return next(s for s in SR.SCENES if s.name == name)


def scratch_row_bytes(capacity):
    return capacity * SCRATCH_BYTES_PER_CONTACT


CROWD = SimpleNamespace(name='crowd-256', N=256, launches=5, substeps=10)       # tests/test_state_isolation_gpu.py: crowd_scene, solver_mode 3


def _step_row(name, scene, kw, sleeps, tensor, row_bytes, boundary, masked, banded=('scratch',)):
    return SimpleNamespace(name=name, scene=scene, kw=kw, sleeps=sleeps, tensor=tensor, row_bytes=row_bytes, boundary=boundary,
                           E=batch_envs(row_bytes, boundary), masked=masked, banded=banded)


_BIG = dict(contact_capacity=MAX_CAPACITY, solver_mode=0)
STEP_ROWS = [
    # the generic kernel, R3 and R2: the global slice of scratch is read and written
    _step_row('scratch-200-p014', _regime_scene('200-p014'), _BIG, (0, 1), 'scratch', scratch_row_bytes(MAX_CAPACITY), B32, True),
    # 1024 kilobots at this capacity: the capacity of the fixed-size kernel is a compile-time constant, so the handle runs the
    # generic kernel with eight waves
    _step_row('scratch-1024-p022-generic', _regime_scene('1024-p022'), _BIG, (0,), 'scratch', scratch_row_bytes(MAX_CAPACITY), B32, True),
    # ... and the fixed-size kernel at the only capacity it has: its slice is 133 120 bytes, 2^32 is reached at 32270 envs
    _step_row('scratch-1024-p022-fixed', _regime_scene('1024-p022'), dict(contact_capacity=0, solver_mode=0), (0,), 'scratch',
              scratch_row_bytes(FIXED_1024_CAPACITY), B32, True),
    # objects, solver_mode 3: ows_acc and the level-sorted records staged in scratch
    _step_row('scratch-crowd-mode3', CROWD, dict(contact_capacity=MAX_CAPACITY, solver_mode=3, num_objects=4), (0,), 'scratch',
              scratch_row_bytes(MAX_CAPACITY), B32, True),
    # row 2: the packed store itself
    _step_row('store-200-p014', _regime_scene('200-p014'), _BIG, (0,), 'ws_key', 4 * MAX_CAPACITY, B31, False, ('scratch', 'ws_key', 'ws_acc')),
]
STEP_BY_NAME = {r.name: r for r in STEP_ROWS}
STEP_CASES = [(r, sl) for r in STEP_ROWS for sl in r.sleeps]
# the 2^32-byte boundary of ws_key / ws_acc: 16385 envs and more of 65528 contacts, i.e. 32 GiB of scratch and more
STORE_B32_ENVS = batch_envs(4 * MAX_CAPACITY, B32)
CONTACTS_K = 8


def step_case_id(case):
    return '%s-%s' % (case[0].name, 'sleep' if case[1] else 'nosleep')


def step_config_kw(row, allow_sleep):
    return dict(row.kw, allow_sleep=allow_sleep)


def step_start(row):
    """(xy [D, N, 2] metres, th [D, N], objects [D, M, 2] metres or None) of the D distinct envs"""
    if row.scene is CROWD:
        xy, _ = scenes.gaussian_spawn(D, CROWD.N, sigma=0.3, seed=61)
        return xy, scenes.toward_objects_theta(xy), np.tile(scenes.CFG4_OBJECTS[None], (D, 1, 1))
    xy, th = SR.start(row.scene, D)
    return xy, th, None


def step_launches(row):
    """[(substeps, actions [D, N, 2])]: what the scene runs, launch by launch"""
    if row.scene is CROWD:
        a = np.zeros((D, CROWD.N, 2), np.float32)
        a[..., 0] = 0.01
        return [(CROWD.substeps, a)] * CROWD.launches
    return [(1, SR.actions(D, row.scene.N, k)) for k in range(row.scene.substeps)]


# the spawn of the masked reset: wide enough that 1024 kilobots neither run out of warm-start slots nor of the 4160 contacts of
# the fixed-size kernel (at 0.1 m they do, and a flagged env has nothing to compare)
RESET_SEED, RESET_STD = 6, 0.4


def step_oracle(row, allow_sleep):
    """The D distinct envs on the oracle at their start."""
    xy, th, objs = step_start(row)
    kw = step_config_kw(row, allow_sleep)
    kw.pop('num_objects', None)
    if objs is not None:
        kw['num_objects'] = objs.shape[-2]
    o = O.OracleSim(O.default_config(D, row.scene.N, **kw))
    o.set_poses_m(xy, th)
    if objs is not None:
        o.set_objects_m(objs)
    return o


def step_need(row):
    """Device bytes of a step row: scratch as the sim allocates it and once more behind its band, the store (twice where it
    is banded, and once for the snapshot of the masked part), a few state tensors of N floats per env."""
    N, cap = row.scene.N, row.row_bytes // SCRATCH_BYTES_PER_CONTACT if row.tensor == 'scratch' else MAX_CAPACITY
    store = 2 * 4 * cap * row.E
    need = 2 * row.E * cap * SCRATCH_BYTES_PER_CONTACT + FRONT_BAND + store * (2 if row.masked else 1) + 24 * 4 * N * row.E
    if 'ws_key' in row.banded:
        need += store + 2 * FRONT_BAND
    return need


# ---- row 3 to 6: sensing, field and render ----------------------------------------------------------------------------------
N_SENSE = MAX_BOTS
RADIUS = RS.RADIUS
NEIGHBORS_K, HIST, RAYS = MAX_NEIGHBORS, (8, 8), (0.2, MAX_RAYS)
GRID = (GRID_MAX_SIDE, GRID_MAX_SIDE)
FIELD_CHANNELS, FIELD_ITERS, FIELD_KEEP, FIELD_SPREAD = FIELD_MAX_CHANNELS, 3, (0.95, 0.8, 0.9, 1.0), (0.2, 0.1, 0.25, 0.05)
FIELD_MASK = RS.FIELD_MASK                  # scene 3 is masked off
GRID_CHANNELS = 1 + 2 + RS.BOXES['num_objects']
E_SENSE = batch_envs(4 * 4 * NEIGHBORS_K * N_SENSE, B32)         # the rows of 256 KiB: 16390
EDGE_RADII = (0.07, 0.1, 0.15, 0.2)
EDGES_MIN_NNZ = 1 << 28                     # 16 bytes of rel per edge: rel passes 2^32 bytes, src and dst 2^30

RENDER_N, RENDER_SIDE = 64, RENDER_MAX_SIDE
RENDER_ROW = 3 * RENDER_SIDE * RENDER_SIDE
E_RENDER = batch_envs(RENDER_ROW, B32)
RENDER_BANDS = tuple(range(0, 64)) + tuple(range(RENDER_SIDE // 2 - 32, RENDER_SIDE // 2 + 32)) + tuple(range(RENDER_SIDE - 64, RENDER_SIDE))

# name; the KilobotSim method; outputs: (name, bytes of one env's row); claims: the output whose rows cross, the boundary
Sensing = collections.namedtuple('Sensing', ('name', 'method', 'outputs', 'claims', 'boundary', 'E'))


def _f(n):
    return 4 * n


def _sensing(name, method, outputs, claims, boundary, E=None):
    row = dict(outputs)[claims]
    return Sensing(name, method, outputs, claims, boundary, batch_envs(row, boundary) if E is None else E)


N_ = N_SENSE
CROSSING = [
    _sensing('neighbors', 'neighbors', (('index', _f(N_ * NEIGHBORS_K)), ('rel', _f(N_ * NEIGHBORS_K * 4)), ('count', _f(N_))), 'rel', B32),
    _sensing('histogram', 'neighbor_histogram', (('hist', _f(N_ * HIST_MAX_BINS)), ('count', _f(N_))), 'hist', B32),
    _sensing('field_step', 'field_step', (('field', _f(FIELD_CHANNELS * GRID[0] * GRID[1])), ('sense', _f(N_ * FIELD_CHANNELS * 4))), 'field', B32),
    # (its rows are larger: 13115 envs would do; it runs on the handle of the others)
    _sensing('grid', 'occupancy_grid', (('grid', _f(GRID_CHANNELS * GRID[0] * GRID[1])),), 'grid', B32),
    _sensing('rays', 'rays', (('dist', _f(N_ * MAX_RAYS)), ('hit', _f(N_ * MAX_RAYS))), 'dist', B31),
    _sensing('render', 'render', (('rgb', RENDER_ROW),), 'rgb', B32),
]
CROSSING_BY_NAME = {r.name: r for r in CROSSING}
# the scene has two objects: obj is [N, 2, 4], 32 KiB per env and 0.5 GiB on this batch, which reaches neither boundary; with
# eight objects it would be 128 KiB like rays.  It runs with the replica relation and the restatement of the distinct envs.
OBJECT_POINTS = _sensing('object_points', 'object_points', (('obj', _f(N_ * RS.BOXES['num_objects'] * 4)), ('wall', _f(N_ * 4))), 'obj', B31, E=E_SENSE)
# edges is ragged: its size follows from the degree sums of the distinct envs (edges_radius)
EDGES = Sensing('edges', 'edges', (('src', None), ('dst', None), ('rel', None), ('offsets', _f(2 * N_)), ('count', _f(N_))), 'rel', B32, E_SENSE)

# The entries whose per-env rows stay below 128 KiB whatever their arguments: name -> (method, the largest row of one env in
# bytes at 1024 kilobots).  They would need more than 32768 envs of 1024 kilobots to pass 2^31 bytes.
_PLANE = _f(GRID_MAX_SIDE * GRID_MAX_SIDE)
CANNOT_CROSS = {
    'sense': ('sense', _f(N_)),
    'reduce-sum': ('neighbor_reduce', _f(N_ * REDUCE_MAX_CHANNELS)),
    'reduce-min': ('neighbor_reduce', _f(N_ * REDUCE_MAX_CHANNELS)),
    'hops': ('hops', _f(N_)),
    'clusters': ('clusters', _f(N_ * 4)),
    'coverage': ('coverage', max(_PLANE, _f(N_ * 4))),
    'paths': ('paths', max(_PLANE, _f(N_ * 4))),
    'targets': ('targets', _f(N_ * 4)),
    'light_sense': ('light_sense', _f(N_)),
    'poses': ('poses', _f(N_ * 3)),
    'host_state': ('host_state', _f(3 * (N_ + MAX_OBJECTS) + 1)),
    'set_actions': ('set_actions', _f(N_ * 2)),
    'reset': ('reset', _f(N_)),
}
CANNOT_CROSS_LIMIT = 128 << 10
# the launching methods that the step rows run
STEP_METHODS = ('step', 'reset_envs', 'contacts', 'reset')


def first_crossing_envs(row_bytes, boundary=B31):
    """The least number of envs at which a tensor of row_bytes per env has a byte at the boundary."""
    return boundary // row_bytes + 1


def table_methods():
    return sorted({r.method for r in CROSSING} | {OBJECT_POINTS.method, EDGES.method} | {m for m, _ in CANNOT_CROSS.values()} | set(STEP_METHODS))


def sensing_need(row):
    """Device bytes of the outputs of a crossing row, each behind its front band, and of the input it tiles (field_step)."""
    need = sum(FRONT_BAND + b * row.E for _, b in row.outputs)
    if row.name == 'field_step':
        need += _f(N_ * FIELD_CHANNELS) * row.E
    return need


def sensing_sim_need(E, N):
    """... and of the sim they run on: two boxes and a light, the default capacity of such a handle."""
    cap = 4 * N + 64 + 40 * RS.BOXES['num_objects']
    return E * (cap * (SCRATCH_BYTES_PER_CONTACT + 8) + 30 * 4 * N)


def edges_radius(degree_sums, E=E_SENSE):
    """The smallest radius whose edge list has at least 2^28 edges plus one env's.  degree_sums: {radius: [D] edges of the
    distinct envs}.  Returns (radius, nnz of the batch)."""
    for R in EDGE_RADII:
        nnz = sum(int(v) for v in degree_sums[R]) * (E // D)
        if nnz >= EDGES_MIN_NNZ + max(int(v) for v in degree_sums[R]):
            return R, nnz
    raise AssertionError('no radius of %s gives 2^28 edges on %d envs' % (EDGE_RADII, E))


def edges_need(nnz):
    return 3 * FRONT_BAND + 24 * nnz + 8 * (E_SENSE * N_SENSE + 1) + 3 * 4 * 4 * (nnz // 16)


# ---- the inputs and the restatements: numpy on the state of the D distinct envs ---------------------------------------------
@functools.lru_cache(maxsize=None)
def field_inputs():
    """(field [D, C, gh, gw], amount [D, N, C]) of the distinct envs"""
    rng = np.random.RandomState(41)
    gw, gh = GRID
    shape = (D, FIELD_CHANNELS, gh, gw)
    field = (rng.uniform(0.25, 1.5, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    return field, rng.uniform(-2.0, 2.0, (D, N_SENSE, FIELD_CHANNELS)).astype(np.float32)


def sensing_config(n, E=D):
    """The native configuration of the sensing handle: what the restatements take their geometry from."""
    from gym_kilobots_amd import _native as nat
    return nat.default_config(E, n, O.DRIVE_VELOCITY, O.LIGHT_CIRCULAR, **RS.config_kw())


def tables_of(cfg):
    """objects_ref.tables of a handle made of cfg -- no device needed."""
    import ctypes as C
    from gym_kilobots_amd import _native as nat
    from tests import objects_ref
    lib, h = nat.load(), C.c_void_p()
    nat.call(lib, 'kb_create', C.byref(cfg), C.byref(h))
    try:
        return objects_ref.tables(nat.outline(h))
    finally:
        lib.kb_destroy(h)


def want(name, tab, st, sentinel_rows=None):
    """The restatement of every output of crossing row `name`, in the row's order, on the state st = (x, y, theta, ox, oy,
    otheta) [D, ...] float32.  sentinel_rows: what the sense output of field_step held before the call."""
    from gym_kilobots_amd import _native as nat
    x, y, th = st[:3]
    if name == 'neighbors':
        from tests import sensing_checks as SC
        return SC.restate_neighbors(x, y, th, RADIUS, NEIGHBORS_K)[:3]
    if name == 'histogram':
        from tests import histogram_ref
        return histogram_ref.restate(x, y, th, RADIUS, HIST[0], HIST[1])
    if name == 'field_step':
        from tests import field_ref
        field, amount = field_inputs()
        return field_ref.restate(tab, field, x, y, th, amount, FIELD_KEEP, FIELD_SPREAD, FIELD_ITERS, FIELD_MASK, fill=sentinel_rows)
    if name == 'grid':
        from tests import grid_ref
        return (grid_ref.restate(tab, GRID[0], GRID[1], grid_ref.ALL, *st),)
    if name == 'rays':
        from tests import rays_ref
        return rays_ref.restate(tab, *st, RAYS[0], 0.0165, RAYS[1], nat.RAY_BOTS | nat.RAY_WALLS | nat.RAY_OBJECTS)
    if name == 'object_points':
        from tests import objects_ref
        return objects_ref.restate(tab, *st)[:2]
    raise KeyError(name)


def want_render_bands(tab, st, lights_m, bot_radius=0.0165):
    """[D, len(RENDER_BANDS), side, 3] uint8: rows RENDER_BANDS of the frames of the distinct envs.  A 2048 x 2048 frame takes
    the restatement several seconds; the 64 rows at the top, in the middle and at the bottom take a tenth of that."""
    from tests import render_ref
    x, y, th, ox, oy, oth = st
    rows = np.array(RENDER_BANDS)
    return np.stack([render_ref.restate_env(tab, RENDER_SIDE, RENDER_SIDE, render_ref.ALL, bot_radius, x[e], y[e], th[e], ox[e], oy[e], oth[e],
                                            ([RS.LIGHT_RADIUS], lights_m[e, :1], lights_m[e, 1:]), rows=rows) for e in range(D)])


OBJ_LIST = 64               # kb_launch.h: the kilobots that may touch one fixture at a time; one more sets status bit 4 on the device


def sensing_oracle(n=N_SENSE):
    """The distinct envs of the sensing rows on the oracle: residency_scenes.spawn(n) with its boxes and lights, as spawned.  The
    six substeps of the residency module are left out at 1024 kilobots: in the first of them up to 82 kilobots lie on one box,
    the device keeps 64 per fixture and flags every env (a staging limit the oracle does not have), and a flagged env drops
    contacts in the order its atomics fall, so its replicas have nothing to be compared by.  No sensing, field or render entry
    reads anything but the poses."""
    xy, th, objs, _ = RS.spawn(n)
    o = O.OracleSim(O.default_config(D, n, O.DRIVE_VELOCITY, O.LIGHT_CIRCULAR, **RS.config_kw()))
    o.set_poses_m(xy, th)
    o.set_objects_m(objs)
    o.light_x[...], o.light_y[...] = RS.LIGHTS_M[:, 0], RS.LIGHTS_M[:, 1]
    return o


def oracle_state(o):
    return tuple(np.array(getattr(o, f)) for f in ('x', 'y', 'theta', 'ox', 'oy', 'otheta'))
