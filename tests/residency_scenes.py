"""The sensing, field and render kernels on a batch that fills the machine more than once: the scene, the batch size and the
table of the sensors.  Needs neither torch nor a device to import; what touches the device imports torch when it is called.

Every other sensing test runs at most eight envs: one workgroup per env (or a few bands per env) on a device with hundreds
of CUs, so every workgroup ever compared ran alone on its CU in the first and only generation of its launch.  Here D = 5
distinct envs are tiled to twice the workgroups the device can hold at once and every replica must give the bits of the
first five, which in turn are held to the restatements (tests/test_sensing_residency_gpu.py).  D is odd because residency
figures are powers of two: with an even D the workgroup that inherits a slot, and the LDS in it, would tend to carry the
same scene as the one before it.

Shared by tests/test_sensing_residency_cpu.py (the scene on the oracle, the batch size, the table against KilobotSim) and
tests/test_sensing_residency_gpu.py."""
import collections
import functools

import numpy as np

from oracle import oracle as O
from tests import scenes
from tests import variant_census as VC

D, N = 5, 333               # N: the suite's partial-tile size at which a lane owns two kilobots
N_PATHS = 64                # ... of the pair that runs kb_sense_paths above the default LDS limit
SIGMA, SPAWN_SEED, ACTION_SEED, SUBSTEPS = 0.2, 17, 18, 6
RADIUS = 0.07
# the two boxes of tests/test_state_isolation_gpu.py (BOXES; that module needs torch), held equal by the CPU test
BOXES = dict(num_objects=2, obj_shape=[O.SHAPE_BOX] * 2 + [0] * 6, obj_nverts=[4] * 2 + [0] * 6,
             obj_verts=[[[0.075 * 25.0, 0.05 * 25.0]] + [[0.0, 0.0]] * 3] * 2 + [[[0.0, 0.0]] * 4] * 6)
LIGHT_RADIUS = 0.3
LIGHTS_M = np.array([[-0.3, 0.2], [0.1, -0.25], [0.35, 0.1], [-0.1, -0.05], [0.2, 0.3]], dtype=np.float32)      # one per distinct env

WAVES_PER_CU = 32           # the hardware's bound on resident waves of a CU, whatever the kernel
WAVE = 64
LDS_CU = 160 * 1024


def config_kw():
    return dict(BOXES, allow_sleep=0, light_radius=LIGHT_RADIUS)


def spawn(n=N):
    """(xy [D, n, 2] metres, th [D, n], objects [D, 2, 2] metres, actions [D, n, 2])"""
    xy, th = scenes.gaussian_spawn(D, n, sigma=SIGMA, seed=SPAWN_SEED)
    return xy, th, np.tile(VC.OBJECTS[None], (D, 1, 1)), scenes.random_actions(D, n, seed=ACTION_SEED)


def oracle_run(n=N, light=O.LIGHT_CIRCULAR):
    """The distinct scene on the oracle after its six substeps."""
    xy, th, objs, a = spawn(n)
    o = O.OracleSim(O.default_config(D, n, O.DRIVE_VELOCITY, light, **config_kw()))
    o.set_poses_m(xy, th)
    o.set_objects_m(objs)
    o.light_x[...], o.light_y[...] = LIGHTS_M[:, 0], LIGHTS_M[:, 1]
    for _ in range(SUBSTEPS):
        o.set_actions(a)
        o.step(1)
    return o


# ---- the batch ------------------------------------------------------------------------------------------------------------
def resident_workgroups(cus, threads=256):
    """An upper bound on the workgroups of `threads` threads that the device holds at once: 32 waves per CU.  LDS and registers
    only lower it, so no occupancy query of the kernel under test is needed."""
    return cus * (WAVES_PER_CU * WAVE // threads)


def resident_by_lds(cus, image_bytes):
    """The same for a kernel whose workgroup takes at least image_bytes of the CU's LDS."""
    return cus * (LDS_CU // image_bytes)


def batch_envs(resident):
    """The smallest multiple of D with at least twice the resident workgroups."""
    return D * -(-2 * resident // D)


# ---- the inputs -----------------------------------------------------------------------------------------------------------
GRID = (64, 48)
PATHS_BIG_GRID = (128, 128)         # tests/test_paths_gpu.py restates it; the plane alone is the default limit of 64 KiB
FIELD_CHANNELS, FIELD_ITERS, FIELD_KEEP, FIELD_SPREAD = 2, 3, (0.95, 0.8), (0.2, 0.1)
FIELD_MASK = np.array([1, 1, 1, 0, 1], dtype=np.uint8)
REDUCE_CHANNELS = 3
TARGET_SLOTS, TARGET_TOL = 40, 0.02
ASSIGN_CUTOFF = 0.25        # metres: the slots in the corners of the table find no kilobot within it and stay unmatched
CLEARANCE = 0.0165
RAYS = (0.2, 16)
NEIGHBORS_K, HIST, CONTACTS_K = 8, (4, 8), 8


@functools.lru_cache(maxsize=None)
def inputs(n=N):
    """{name: array [D, ...]}: what the sensors take besides the state, one row per distinct env."""
    from tests import paths_ref
    rng = np.random.RandomState(31)
    gw, gh = GRID
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)      # noqa: E731
    v = dict(messages=f32(rng.uniform(-4.0, 4.0, (D, n, REDUCE_CHANNELS))),
             seeds=((np.arange(n)[None, :] + np.arange(D)[:, None]) % 7 == 0).astype(np.uint8),
             field=f32(rng.uniform(0.25, 1.5, (D, FIELD_CHANNELS, gh, gw)) * rng.choice([-1.0, 1.0], (D, FIELD_CHANNELS, gh, gw))),
             amount=f32(rng.uniform(-2.0, 2.0, (D, n, FIELD_CHANNELS))),
             field_mask=FIELD_MASK,
             points=f32(rng.uniform(-1.0, 1.0, (D, TARGET_SLOTS, 2)) * [0.9, 0.65]),
             light_action=f32(rng.uniform(-0.01, 0.01, (D, 2))))
    v['source'], v['blocked'] = paths_ref.random_masks(D, gw, gh, seed=37, density=0.1)
    # the raised-limit grid: env 0 carries the serpentine, whose sweep count is far beyond gw + gh
    bw, bh = PATHS_BIG_GRID
    v['source_big'], v['blocked_big'] = paths_ref.random_masks(D, bw, bh, seed=38, density=0.1)
    v['blocked_big'][0], v['source_big'][0] = paths_ref.serpentine(bw, bh), paths_ref.mask_of(bw, bh, [(0, 0)])
    return v


def tiled(sim, name):
    """Input `name` for every env of the sim, on its device: row e is the distinct row e % D.  Uploaded once per sim."""
    import torch
    cache = sim.__dict__.setdefault('_residency_inputs', {})
    if name not in cache:
        a = inputs(sim.num_bots)[name]
        reps = sim.num_envs // D
        assert reps * D == sim.num_envs
        cache[name] = torch.from_numpy(np.ascontiguousarray(np.tile(a, (reps,) + (1,) * (a.ndim - 1)))).to(sim.device)
    return cache[name]


# ---- the sensors ----------------------------------------------------------------------------------------------------------
# name; the KilobotSim method; the names of the outputs; call(sim, out) -> the output tensors in that order, into `out` (what an
# earlier call returned) if it is given; few: outputs that are per-env statistics of few values, of which the distinct envs
# need only be not all equal
Row = collections.namedtuple('Row', ('name', 'method', 'outputs', 'call', 'few'))


def _first(out):
    return None if out is None else out[0]


def _edges(sim, out):
    e = sim.edges(RADIUS, out=None if out is None else out[:3])
    return e.src, e.dst, e.rel, e.offsets, e.count


def _reduce(op):
    def call(sim, out):
        return sim.neighbor_reduce(tiled(sim, 'messages'), RADIUS, op=op, out=out, count=True)
    return call


def _field(sim, out):
    import torch
    field = tiled(sim, 'field').clone() if out is None else out[0].copy_(tiled(sim, 'field'))
    sense = torch.zeros(sim.num_envs, sim.num_bots, FIELD_CHANNELS, 4, device=sim.device) if out is None else out[1].zero_()
    sim.field_step(field, tiled(sim, 'amount'), FIELD_KEEP, FIELD_SPREAD, FIELD_ITERS, tiled(sim, 'field_mask'), out=sense)
    return field, sense


def _paths(grid, suffix=''):
    def call(sim, out):
        return tuple(sim.paths(grid[0], grid[1], tiled(sim, 'source' + suffix), tiled(sim, 'blocked' + suffix), objects='all', clearance_m=CLEARANCE, out=out))
    return call


def _light_sense(sim, out):
    """The first call moves the light; the repeat leaves it where it is and senses again."""
    sim.light_sense(tiled(sim, 'light_action') if out is None else None)
    return sim.light_value, sim.light_gx, sim.light_gy, sim.light_x, sim.light_y


SENSORS = [
    Row('sense', 'sense', ('count',), lambda sim, out: (sim.sense(RADIUS, out=_first(out)),), ()),
    Row('neighbors', 'neighbors', ('index', 'rel', 'count'), lambda sim, out: sim.neighbors(RADIUS, NEIGHBORS_K, out=out), ()),
    Row('edges', 'edges', ('src', 'dst', 'rel', 'offsets', 'count'), _edges, ()),
    Row('histogram', 'neighbor_histogram', ('hist', 'count'), lambda sim, out: sim.neighbor_histogram(RADIUS, HIST[0], HIST[1], out=out, count=True), ()),
    Row('reduce-sum', 'neighbor_reduce', ('result', 'count'), _reduce('sum'), ()),
    Row('reduce-min', 'neighbor_reduce', ('result', 'count'), _reduce('min'), ()),
    Row('hops', 'hops', ('hops', 'parent', 'root', 'stats'),
        lambda sim, out: sim.hops(tiled(sim, 'seeds'), RADIUS, parent=True, root=True, stats=True, out=out), ('stats',)),
    Row('clusters', 'clusters', ('label', 'size', 'table', 'stats'), lambda sim, out: sim.clusters(RADIUS, size=True, table=True, stats=True, out=out), ('stats',)),
    Row('rays', 'rays', ('dist', 'hit'), lambda sim, out: sim.rays(RAYS[0], RAYS[1], out=out), ()),
    Row('object_points', 'object_points', ('obj', 'wall'), lambda sim, out: sim.object_points(out=out), ()),
    Row('grid', 'occupancy_grid', ('grid',), lambda sim, out: (sim.occupancy_grid(GRID[0], GRID[1], ('count', 'flow', 'objects'), out=_first(out)),), ()),
    Row('coverage', 'coverage', ('owner', 'dist', 'cells', 'stats'), lambda sim, out: tuple(sim.coverage(GRID[0], GRID[1], out=out)), ()),
    Row('field_step', 'field_step', ('field', 'sense'), _field, ()),
    Row('paths', 'paths', ('dist', 'step', 'bots', 'stats'), _paths(GRID), ()),
    Row('targets', 'targets', ('index', 'rel', 'owner', 'dist', 'stats'), lambda sim, out: tuple(sim.targets(tiled(sim, 'points'), TARGET_TOL, out=out)), ()),
    Row('assign', 'targets', ('index', 'rel', 'owner', 'dist', 'stats'),
        lambda sim, out: tuple(sim.targets(tiled(sim, 'points'), TARGET_TOL, out=out, match='greedy', cutoff_m=ASSIGN_CUTOFF)), ()),
    Row('contacts', 'contacts', ('partner', 'impulse', 'touch', 'obj'), lambda sim, out: sim.contacts(CONTACTS_K, out=out), ()),
    Row('render', 'render', ('rgb',), lambda sim, out: (sim.render(GRID[0], GRID[1], out=_first(out)),), ()),
    Row('light_sense', 'light_sense', ('light_value', 'light_gx', 'light_gy', 'light_x', 'light_y'), _light_sense, ()),
]
BY_NAME = {row.name: row for row in SENSORS}
# kb_sense_paths with an LDS image above 64 KiB, which changes how many workgroups a CU takes: on a pair of its own
PATHS_BIG = Row('paths-128', 'paths', ('dist', 'step', 'bots', 'stats'), _paths(PATHS_BIG_GRID, '_big'), ())
