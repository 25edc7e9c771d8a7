"""Scenes off the default arena and the default constants, shared by tests/test_geometry_cpu.py (the claims of every row
hold on the host, and no scene is vacuous on the oracle), tests/test_geometry_gpu.py (every row bit for bit against the
oracle) and tests/test_sensing_geometry_gpu.py (the sensing kernels on the same grids).

kb_create derives the broadphase grid from world_width, world_height and bot_radius: the cell starts at 0.875 world units
and doubles while it is below the kilobot diameter and while the grid has more than 8192 cells.  From the cell count follow
the cell heads (direct or hashed), the whole LDS image and -- in the sorted-bin kernels with the sleep state -- where the
per-island minimum of the sleep times lies (kb_launch.h: bins_image):

    branch 1   over the bin boundaries        binE_size(nhead, nw) >= 4 NB
    branch 2   over the staged pairs          else capL >= NB
    branch 3   behind the image               else

GEOMETRY is the table of arenas and radii, CONSTANTS the table of scene constants moved off their defaults."""
from types import SimpleNamespace

import numpy as np

from oracle import oracle as O
from tests import scenes
from tests.scenes import put_numpy  # noqa: F401

E = 2
WORLD_SCALE, CELL_SIZE, MAX_CELLS = 25.0, 0.875, 8192         # kb_common.h
R_DEFAULT = 0.0165
PITCH = 0.97                # lattice pitch in kilobot diameters: neighbours overlap by 3 % and touch from the first substep
JITTER = 0.03               # ... and the jitter, in diameters: pitch -+ jitter stays within 0.95 .. 1.0 diameters on average
PLANTED = 12                # kilobots against the walls (two per wall) and in the corners
WALL_DEPTH = 0.97           # their distance from the wall in radii
SINGLE_SUBSTEPS, FUSED_SUBSTEPS, REST_SUBSTEPS, WAKE_SUBSTEPS = 3, 10, 6, 2
MODE_DENSITY = [2.0, 2.0, 1.0, 1.0, 1.0]

BOT_FIELDS = ('x', 'y', 'theta', 'cmd_vx', 'cmd_vy', 'cmd_w', 'status')
OBJ_FIELDS = ('ox', 'oy', 'otheta', 'ovx', 'ovy', 'ow', 'ows_acc')


def grid(W, H, r):
    """(cell size in world units, gw, gh) by the fp32 expressions of kb_create (kb_abi.hip)."""
    f = np.float32
    Ww, Hw = f(W) * f(WORLD_SCALE), f(H) * f(WORLD_SCALE)
    cell = f(CELL_SIZE)
    dmin = f(2.0) * f(r) * f(WORLD_SCALE)
    while cell < dmin:
        cell = cell * f(2.0)
    while True:
        inv = f(1.0) / cell
        gw = max(int(np.ceil(Ww * inv)), 1)
        gh = max(int(np.ceil(Hw * inv)), 1)
        if gw * gh <= MAX_CELLS:
            return float(cell), gw, gh
        cell = cell * f(2.0)


# ---- the geometry table ------------------------------------------------------------------------------------------------
#   family   'bins' (sorted-bin kernels: velocity drive, no objects), 'objects' (a box and a disc), 'mixed' (KB_DRIVE_MIXED)
#   cell, gw, gh, hashed, branch, fn: what the row claims of kb_create and plan_launch (branch 0: the kernel has no islMin,
#   i.e. no sleep state or not a sorted-bin kernel; fn: 1024 for the fixed-size instantiation)
#   objscale: the objects are a 0.15 x 0.10 m box and a disc of radius 0.06 m, times this
def _G(name, W, H, r, N, sleep, cell, gw, gh, hashed, branch, fn, what, family='bins', objscale=1.0, pitch=PITCH):
    g = SimpleNamespace(name=name, W=W, H=H, r=r, N=N, sleep=sleep, cell=cell, gw=gw, gh=gh, hashed=hashed, branch=branch, fn=fn,
                        what=what, family=family, pitch=pitch, shapes=[], objects=None, ovel=None)
    if family == 'objects':     # the box left and the disc right of the centre, at rest: (x, y, theta) in metres and radians
        d = 0.18 * objscale + 2.0 * r
        g.shapes = [('box', 0.15 * objscale, 0.10 * objscale), ('circle', 0.06 * objscale)]
        g.objects = np.array([[-d, 0.0, 0.3 if H > 0.1 else 0.0], [d, 0.0, 0.0]])
        g.ovel = np.zeros((2, 3), np.float32)
    return g


GEOMETRY = [
    # 1.6 x 1.2 m: 1610 cells, below the ~2070 at which the bin boundaries stop covering islMin
    # (888: eight waves' bucket tables still cover islMin; under kb_set_block_threads(448) they do not -- the only way to
    #  another width off the bin boundaries, since 2 * 448 < 977)
    _G('1.6x1.2-888-sleep', 1.6, 1.2, R_DEFAULT, 888, 1, 0.875, 46, 35, 0, 1, 0, 'islMin over the staged pairs at a second width'),
    _G('1.6x1.2-1000-sleep', 1.6, 1.2, R_DEFAULT, 1000, 1, 0.875, 46, 35, 0, 2, 0, 'islMin over the staged pairs'),
    _G('1.6x1.2-1022-sleep', 1.6, 1.2, R_DEFAULT, 1022, 1, 0.875, 46, 35, 0, 3, 0, 'islMin behind the image'),
    _G('1.6x1.2-1024', 1.6, 1.2, R_DEFAULT, 1024, 0, 0.875, 46, 35, 0, 0, 1024, 'fixed-size kernel on a small bin table'),
    _G('1.6x1.2-1024-sleep', 1.6, 1.2, R_DEFAULT, 1024, 1, 0.875, 46, 35, 0, 3, 1024, 'fixed-size kernel, islMin past its bin table'),
    # 3.6 x 2.7 m: 8034 cells, the largest grid at cell 0.875
    _G('3.6x2.7-200-sleep', 3.6, 2.7, R_DEFAULT, 200, 1, 0.875, 103, 78, 1, 1, 0, 'hashed bins in a large arena'),
    _G('3.6x2.7-700-sleep', 3.6, 2.7, R_DEFAULT, 700, 1, 0.875, 103, 78, 1, 1, 0, 'hashed bins above 512 kilobots'),
    _G('3.6x2.7-1022-sleep', 3.6, 2.7, R_DEFAULT, 1022, 1, 0.875, 103, 78, 1, 3, 0, 'islMin behind the image with hashed bins'),
    _G('3.6x2.7-1024-sleep', 3.6, 2.7, R_DEFAULT, 1024, 1, 0.875, 103, 78, 0, 1, 1024, 'the largest direct bin table, multi-chunk scan'),
    # 4.0 x 2.9 m: 115 x 83 = 9545 cells of 0.875 are more than MAX_CELLS
    _G('4.0x2.9-200', 4.0, 2.9, R_DEFAULT, 200, 0, 1.75, 58, 42, 1, 0, 0, 'cell doubled by the MAX_CELLS loop'),
    _G('4.0x2.9-1024-sleep', 4.0, 2.9, R_DEFAULT, 1024, 1, 1.75, 58, 42, 0, 1, 1024, 'cell doubled by the MAX_CELLS loop, fixed-size kernel'),
    # corridors: the stencil is clipped on both sides
    _G('2.0x0.06-40', 2.0, 0.06, R_DEFAULT, 40, 0, 0.875, 58, 2, 0, 0, 0, 'two-row grid'),
    _G('2.0x0.06-40-sleep', 2.0, 0.06, R_DEFAULT, 40, 1, 0.875, 58, 2, 0, 1, 0, 'two-row grid'),
    _G('0.06x1.5-40', 0.06, 1.5, R_DEFAULT, 40, 0, 0.875, 2, 43, 0, 0, 0, 'two-column grid'),
    _G('0.06x1.5-40-sleep', 0.06, 1.5, R_DEFAULT, 40, 1, 0.875, 2, 43, 0, 1, 0, 'two-column grid'),
    # (at 0.034 m the walls are 0.85 world units apart and a kilobot reaches 0.4225 from its centre: it touches one wall at
    #  a time; at 0.0335 m it touches both, 0.00375 deep each, which is inside the linear slop and stays)
    _G('2.0x0.034-40', 2.0, 0.034, R_DEFAULT, 40, 0, 0.875, 58, 1, 0, 0, 0, 'one-row grid, kilobots between two walls'),
    _G('2.0x0.034-40-sleep', 2.0, 0.034, R_DEFAULT, 40, 1, 0.875, 58, 1, 0, 1, 0, 'one-row grid, kilobots between two walls'),
    _G('2.0x0.0335-40', 2.0, 0.0335, R_DEFAULT, 40, 0, 0.875, 58, 1, 0, 0, 0, 'one-row grid, every kilobot on two walls'),
    _G('2.0x0.0335-40-sleep', 2.0, 0.0335, R_DEFAULT, 40, 1, 0.875, 58, 1, 0, 1, 0, 'one-row grid, every kilobot on two walls'),
    # radii: the cell doubles while it is below the diameter
    _G('r0.02-200', 2.0, 1.5, 0.02, 200, 0, 1.75, 29, 22, 0, 0, 0, 'cell doubled by the radius'),
    _G('r0.02-1000-sleep', 2.0, 1.5, 0.02, 1000, 1, 1.75, 29, 22, 0, 2, 0, 'islMin over the staged pairs at cell 1.75'),
    _G('r0.04-200-sleep', 2.0, 1.5, 0.04, 200, 1, 3.5, 15, 11, 0, 1, 0, 'cell doubled twice'),
    _G('r0.008-200', 2.0, 1.5, 0.008, 200, 0, 0.875, 58, 43, 1, 0, 0, 'crowded bins: five or six kilobots per cell'),
    _G('r0.008-700-sleep', 2.0, 1.5, 0.008, 700, 1, 0.875, 58, 43, 0, 1, 0, 'crowded bins: five or six kilobots per cell'),
    # kernels with the head table in front of the manifold records
    _G('objects-2.0x0.06', 2.0, 0.06, R_DEFAULT, 96, 0, 0.875, 58, 2, 0, 0, 0, 'objects on a two-row grid', 'objects', objscale=0.2),
    _G('objects-r0.02', 2.0, 1.5, 0.02, 96, 0, 1.75, 29, 22, 1, 0, 0, 'objects at cell 1.75', 'objects'),
    _G('objects-3.0x2.0-sleep', 3.0, 2.0, R_DEFAULT, 96, 1, 0.875, 86, 58, 1, 0, 0, 'objects, hashed heads in a large arena', 'objects'),
    _G('mixed-2.0x0.06', 2.0, 0.06, R_DEFAULT, 96, 0, 0.875, 58, 2, 0, 0, 0, 'mixed laws on a two-row grid', 'mixed'),
    _G('mixed-r0.02', 2.0, 1.5, 0.02, 96, 0, 1.75, 29, 22, 1, 0, 0, 'mixed laws at cell 1.75', 'mixed'),
    _G('mixed-3.0x2.0', 3.0, 2.0, R_DEFAULT, 96, 0, 0.875, 86, 58, 1, 0, 0, 'mixed laws, hashed heads in a large arena', 'mixed'),
]

# What the table must keep covering (tests/test_geometry_cpu.py): a predicate over the rows and how many rows must meet it
COVERAGE = [
    ('islMin over the bin boundaries in a sleep row', lambda g: g.sleep and g.branch == 1, 1),
    ('islMin over the staged pairs in a sleep row', lambda g: g.sleep and g.branch == 2, 1),
    ('islMin behind the image in a sleep row', lambda g: g.sleep and g.branch == 3, 1),
    ('hashed bins at cell 0.875', lambda g: g.family == 'bins' and g.hashed and g.cell == 0.875, 1),
    ('direct bins at cell 0.875', lambda g: g.family == 'bins' and not g.hashed and g.cell == 0.875, 1),
    ('hashed bins at cell 1.75', lambda g: g.family == 'bins' and g.hashed and g.cell == 1.75, 1),
    ('direct bins at cell 1.75', lambda g: g.family == 'bins' and not g.hashed and g.cell == 1.75, 1),
    ('hashed bins above 512 kilobots', lambda g: g.family == 'bins' and g.hashed and g.N > 512, 2),
    ('islMin behind the image with hashed bins', lambda g: g.hashed and g.branch == 3, 1),
    ('the fixed-size kernel below 2070 cells', lambda g: g.fn == 1024 and g.gw * g.gh < 2070, 1),
    ('the fixed-size kernel above 4096 cells', lambda g: g.fn == 1024 and g.gw * g.gh > 4096, 1),
    ('the fixed-size kernel with islMin past its bin table', lambda g: g.fn == 1024 and g.sleep and g.branch == 3, 1),
    ('a one-row grid', lambda g: g.gh == 1, 1),
    ('every kilobot on two walls', lambda g: on_two_walls(g), 1),
    ('a two-row grid', lambda g: g.gh == 2 and g.family == 'bins', 1),
    ('a two-column grid', lambda g: g.gw == 2, 1),
    ('cell 3.5', lambda g: g.cell == 3.5, 1),
    ('crowded bins', lambda g: g.r < 0.01, 2),
    ('objects at a non-default cell', lambda g: g.family == 'objects' and g.cell != 0.875, 1),
    ('objects on a two-row grid', lambda g: g.family == 'objects' and g.gh == 2, 1),
    ('mixed laws at a non-default cell', lambda g: g.family == 'mixed' and g.cell != 0.875, 1),
    ('mixed laws on a two-row grid', lambda g: g.family == 'mixed' and g.gh == 2, 1),
]
FIXED_ARENAS = 3            # fn == 1024 occurs in at least this many arenas

# Sleep rows that run again under kb_set_block_threads: (row, width, islMin placement at that width).  A width is a multiple
# of 64 up to 512 that leaves at most two kilobots per thread, so a swarm of more than 896 has one width only.  The rows
# that leave the bin boundaries at kb_create's width are all larger than that; at 448 threads the bucket tables of seven
# waves are smaller and 888 kilobots take placement 2.  Placement 3 needs fewer staged contacts than bodies, which the
# plan reaches only where 512 is the one legal width (tests/test_geometry_cpu.py asserts both).
SECOND_WIDTH = [('3.6x2.7-700-sleep', 448, 1), ('1.6x1.2-888-sleep', 448, 2)]
WIDEST, BOTS_PER_THREAD = 512, 2


def on_two_walls(g):
    """The walls of the narrow side are closer than two contact reaches (radius + b2_polygonRadius): no kilobot fits between
    them without touching both."""
    return min(g.W, g.H) * WORLD_SCALE < 2.0 * (g.r * WORLD_SCALE + 0.01)


def row_id(g):
    return g.name


def plan_inputs(g, threads=0):
    """The eleven inputs of plan_launch (columns of tests/golden/launch_plan.txt) of a geometry or constants row."""
    M = len(g.shapes) if g.family == 'objects' else 0
    drive = O.DRIVE_MIXED if g.family == 'mixed' else O.DRIVE_VELOCITY
    return [g.N, M, M, 0, drive, O.LIGHT_NONE, 0, g.sleep, g.gw * g.gh, 0, threads]


def shapes_kw(shapes):
    """shapes: [('box', width, height) | ('circle', radius)] in metres -> config keywords."""
    kw = dict(num_objects=len(shapes), obj_shape=[], obj_verts=[], obj_radius=[], obj_nverts=[])
    for sh in shapes:
        box = sh[0] == 'box'
        kw['obj_shape'].append(O.SHAPE_BOX if box else O.SHAPE_CIRCLE)
        kw['obj_verts'].append([[sh[1] / 2 * WORLD_SCALE, sh[2] / 2 * WORLD_SCALE]] if box else [[0.0, 0.0]])
        kw['obj_radius'].append(0.0 if box else sh[1])
        kw['obj_nverts'].append(4 if box else 0)
    return kw


def config_kw(g):
    kw = dict(world_width=g.W, world_height=g.H, bot_radius=g.r, allow_sleep=g.sleep)
    if g.family == 'objects':
        kw.update(shapes_kw(g.shapes))
    if g.family == 'mixed':
        kw.update(mode_density=list(getattr(g, 'mode_density', MODE_DENSITY)))
    kw.update(getattr(g, 'constants', {}))
    return kw


# ---- scenes ------------------------------------------------------------------------------------------------------------
def _sites(W, H, r, pitch, groups=False):
    """Lattice sites (metres) at which a kilobot fits the arena, centred: a square lattice; where no second full row fits,
    two staggered rows on the two long walls, stretched so that the diagonal neighbours are one pitch apart (the overlap can
    be pushed out along the corridor), or one row in the middle.  groups: in such a strip, four sites in a row stay and two
    are left out -- islands of four come to rest within a few substeps, a chain of forty does not."""
    if W < H:
        return _sites(H, W, r, pitch, groups)[:, ::-1]
    wu, hu = W - 2.0 * r, H - 2.0 * r           # where centres may lie
    staggered = 0.5 * pitch <= hu < pitch
    px = 2.0 * np.sqrt(pitch * pitch - hu * hu) if staggered else pitch
    nx = int(np.floor(wu / px)) + 1
    xs = (np.arange(nx) - (nx - 1) / 2.0) * px
    if hu >= pitch:
        ny = int(np.floor(hu / pitch)) + 1
        ys = (np.arange(ny) - (ny - 1) / 2.0) * pitch
        gx, gy = np.meshgrid(xs, ys)
        return np.stack([gx.ravel(), gy.ravel()], -1)
    if staggered:
        low = np.stack([xs, np.full(nx, -hu / 2.0)], -1)
        high = np.stack([xs[:-1] + px / 2.0, np.full(nx - 1, hu / 2.0)], -1)
        strip = np.concatenate([low, high])
    else:
        strip = np.stack([xs, np.zeros(nx)], -1)
    strip = strip[np.argsort(strip[:, 0], kind='stable')]
    return strip[np.arange(len(strip)) % 6 < 4] if groups else strip


def _gap(s, pose, sh):
    """Distance (metres) of the points s [n, 2] from the outline of an object at pose (x, y, theta); 0 inside."""
    dx, dy = s[:, 0] - pose[0], s[:, 1] - pose[1]
    if sh[0] == 'circle':
        return np.maximum(np.hypot(dx, dy) - sh[1], 0.0)
    c, sn = np.cos(pose[2]), np.sin(pose[2])
    lx, ly = c * dx + sn * dy, c * dy - sn * dx
    return np.hypot(np.maximum(np.abs(lx) - sh[1] / 2.0, 0.0), np.maximum(np.abs(ly) - sh[2] / 2.0, 0.0))


def _crowd(g, N, pitch, clear):
    """The N lattice sites nearest the centre of the arena that keep clear of the objects: clear = [(pose, shape)]; a site
    stays if its kilobot overlaps the object by at most a tenth of its radius -- the innermost ring touches the objects."""
    s = _sites(g.W, g.H, g.r, pitch, groups=g.family == 'bins')
    for pose, sh in clear:
        s = s[_gap(s, pose, sh) >= 0.9 * g.r]
    assert len(s) >= N, '%s: %d sites for %d kilobots' % (g.name, len(s), N)
    return s[np.argsort(np.hypot(s[:, 0], s[:, 1]), kind='stable')[:N]]


def start(g, seed=11):
    """Poses of a row: xy [E, N, 2] metres and th [E, N].  A lattice at PITCH diameters with jitter, scaled to the row's
    radius -- scenes.lattice_spawn where its square fits the arena, the sites of the arena nearest the centre otherwise and
    around objects --, clipped to the arena; the last PLANTED kilobots against each wall and in each corner, heading into
    it; then the ids are shuffled per env."""
    N, r = g.N, g.r
    pitch, jitter = g.pitch * 2.0 * r, JITTER * 2.0 * r
    rng = np.random.RandomState(seed)
    side = int(np.ceil(np.sqrt(N)))
    if g.family == 'bins' and (side - 1) * pitch <= min(g.W, g.H) - 2.0 * r:
        xy, th = scenes.lattice_spawn(E, N, seed=seed, pitch=pitch, jitter=jitter)
    else:
        clear = list(zip(g.objects, g.shapes)) if g.family == 'objects' else []
        xy = _crowd(g, N, pitch, clear)[None] + rng.uniform(-jitter, jitter, size=(E, N, 2))
        th = rng.uniform(-np.pi, np.pi, size=(E, N))
    if g.family == 'objects':           # the crowd heads for the nearer of the first two objects
        p = g.objects[:2]
        k = np.argmin(np.hypot(xy[..., None, 0] - p[:, 0], xy[..., None, 1] - p[:, 1]), -1)
        th = np.arctan2(p[k, 1] - xy[..., 1], p[k, 0] - xy[..., 0])
    hx, hy = g.W / 2.0 - WALL_DEPTH * r, g.H / 2.0 - WALL_DEPTH * r
    fx, fy = 0.45 * g.W, 0.45 * g.H             # (outside the lattice, which lies around the centre)
    if N >= 40:
        planted = [(-hx, -fy, np.pi), (-hx, fy, np.pi), (hx, -fy, 0.0), (hx, fy, 0.0),
                   (-fx, -hy, -np.pi / 2), (fx, -hy, -np.pi / 2), (-fx, hy, np.pi / 2), (fx, hy, np.pi / 2),
                   (-hx, -hy, -3 * np.pi / 4), (hx, -hy, -np.pi / 4), (hx, hy, np.pi / 4), (-hx, hy, 3 * np.pi / 4)]
        assert len(planted) == PLANTED
        for i, (px, py, pth) in enumerate(planted):
            xy[:, N - PLANTED + i] = (px, py)
            th[:, N - PLANTED + i] = pth + rng.uniform(-0.3, 0.3, size=E)
    xy[..., 0] = np.clip(xy[..., 0], -hx, hx)
    xy[..., 1] = np.clip(xy[..., 1], -hy, hy)
    for e in range(E):
        perm = rng.permutation(N)
        xy[e], th[e] = xy[e][perm], th[e][perm]
    return xy, th


def scene(g, seed=11):
    """Everything a run of one row needs:
      E, N, mode, kw         arguments of tests.gpu_common.make_pair / oracle.default_config
      xy, th                 kilobot poses
      objects, ovel          object poses [E, M, 3] (metres, radians) and velocities (ovx, ovy, ow) [E, M] each, or None
      state                  {buffer name: array} written into both sims before the first substep (laws, motors)
      launches               [(n_substeps, actions, phase)], phase in 'single', 'fused', 'rest', 'wake'; compare after each
      fields                 what is compared bit for bit after every launch (besides the packed warm-start list)"""
    N = g.N
    s = SimpleNamespace(E=E, N=N, mode=O.DRIVE_MIXED if g.family == 'mixed' else O.DRIVE_VELOCITY, kw=config_kw(g), state={},
                        objects=None, ovel=None)
    s.xy, s.th = start(g, seed)
    rng = np.random.RandomState(seed + 1)
    if g.family == 'objects':
        s.objects = np.tile(np.asarray(g.objects, np.float64)[None], (E, 1, 1))
        s.objects[1, :2, :2] *= 0.99          # the envs differ in the objects inside the crowd too
        s.ovel = tuple(np.tile(np.asarray(g.ovel, np.float32)[None, :, k], (E, 1)) for k in range(3))
    if g.family == 'mixed':
        ml, mr = rng.randint(0, 256, (E, N)).astype(np.uint8), rng.randint(0, 256, (E, N)).astype(np.uint8)
        off = rng.rand(E, N) < 0.3
        ml[off] = 0
        mr[off] = 0
        s.state.update(bot_mode=rng.randint(0, 5, (E, N)).astype(np.uint8), motor_l=ml, motor_r=mr)

    def driven(k):
        a = scenes.random_actions(E, N, seed=seed + 100 + k)
        if g.family == 'objects':
            a[:, ::2] = (0.01, 0.0)             # every second kilobot rams ahead, into the objects
        return a
    s.launches = [(1, driven(k), 'single') for k in range(SINGLE_SUBSTEPS)] + [(FUSED_SUBSTEPS, driven(SINGLE_SUBSTEPS), 'fused')]
    if g.sleep:
        s.launches += [(1, np.zeros((E, N, 2), np.float32), 'rest')] * REST_SUBSTEPS
        for k in range(WAKE_SUBSTEPS):          # every third kilobot starts again and wakes its island
            a = driven(SINGLE_SUBSTEPS + 1 + k)
            a[:, np.arange(N) % 3 != 0] = 0.0
            s.launches.append((1, a, 'wake'))
    s.fields = BOT_FIELDS + (OBJ_FIELDS if g.family == 'objects' else ()) + (('sleep_time',) if g.sleep else ()) \
        + (('osleep',) if g.sleep and g.family == 'objects' else ())
    return s


def apply_start(s, sim, put):
    """Objects and start state of scene s into one sim (the kilobot poses are set before); put(sim, name, array) writes
    one buffer."""
    if s.objects is not None:
        sim.set_objects_m(s.objects[..., :2], s.objects[..., 2])
        for name, val in zip(('ovx', 'ovy', 'ow'), s.ovel):
            put(sim, name, val)
    for name, val in s.state.items():
        put(sim, name, val)


def oracle_sim(s):
    osim = O.OracleSim(O.default_config(s.E, s.N, s.mode, O.LIGHT_NONE, **s.kw))
    osim.set_poses_m(s.xy, s.th)
    apply_start(s, osim, put_numpy)
    return osim


def oracle_contacts(osim):
    """(kilobot-kilobot, wall, kilobot-fixture) contacts of the last substep, the least over the envs."""
    c = np.array([osim.count_contacts(e, True) for e in range(osim.cfg.num_envs)])
    return tuple(int(v) for v in c.min(0))


def _sensing_rows():
    """One row per (arena, radius, swarm size): those of up to 200 kilobots, and 1024 in the 1.6 x 1.2 m and 3.6 x 2.7 m arenas."""
    seen, rows = set(), []
    for g in GEOMETRY:
        key = (g.W, g.H, g.r, g.N)
        if key not in seen and (g.N <= 200 or (g.N == 1024 and g.W in (1.6, 3.6))):
            rows.append(g)
        seen.add(key)
    return rows


SENSING_ROWS = _sensing_rows()      # the rows that the sensing kernels are run on


def sensing_radius(g, kind):
    """metres"""
    cell = g.cell / WORLD_SCALE
    return {'half-cell': 0.5 * cell, 'cell-and-a-half': 1.5 * cell, 'arena': float(np.hypot(g.W, g.H))}[kind]


# ---- the constants table -----------------------------------------------------------------------------------------------
# Three kernels in the default arena at the default radius, allow_sleep 0: the sorted-bin kernel at 200 kilobots, a kernel
# with objects at 96 (the crowd pushes a box and a disc; a second box lies rotated against the bottom wall and is thrown
# along and into it, so the two friction coefficients act on its wall manifold) and the mixed kernel at 96, where the laws
# 2 .. 4 have no density of their own and take bot_density.
#   acts   'bots': the constant must change x / y / theta / ws_acc of the kilobots on the oracle;
#          a tuple of object indices: it must change ox / oy / otheta / ows_acc of at least one of these objects
WALL_BOX = 2
CONSTANT_KERNELS = {
    'bins': dict(N=200, family='bins'),
    'objects': dict(N=96, family='objects'),
    'mixed': dict(N=96, family='mixed'),
}
BOT_CONSTANTS = [
    ('dt-0.05', dict(dt=0.05), 'bots'),
    ('dt-0.15', dict(dt=0.15), 'bots'),
    ('bot-density-0.7', dict(bot_density=0.7), 'bots'),
    ('bot-density-3.5', dict(bot_density=3.5), 'bots'),
    ('bot-linear-damping-0.3', dict(bot_linear_damping=0.3), 'bots'),
    ('bot-angular-damping-2.5', dict(bot_angular_damping=2.5), 'bots'),
    # KB_DAMPING_LINEAR: 1 - 0.1 * 12 and 1 - 0.1 * 15 are negative, the clamp sends both factors to 0
    ('linear-model-clamped', dict(damping_model=1, bot_linear_damping=12.0, bot_angular_damping=15.0), 'bots'),
]
OBJ_CONSTANTS = [
    ('obj-density-0.7', dict(obj_density=0.7), (0, 1)),
    ('obj-friction-0.6', dict(obj_friction=0.6), (WALL_BOX,)),
    ('wall-friction-0.9', dict(wall_friction=0.9), (WALL_BOX,)),
    ('obj-linear-damping-0.2', dict(obj_linear_damping=0.2), (0, 1, WALL_BOX)),
    ('obj-angular-damping-3.0', dict(obj_angular_damping=3.0), (0, WALL_BOX)),
]
ALL_BOT = dict(dt=0.08, bot_density=1.3, bot_linear_damping=0.5, bot_angular_damping=1.7)
ALL_OBJ = dict(obj_density=1.4, obj_friction=0.3, wall_friction=0.5, obj_linear_damping=0.4, obj_angular_damping=1.5)


CONSTANTS_SHAPES = [('box', 0.15, 0.10), ('circle', 0.06), ('box', 0.2, 0.1)]
CONSTANTS_OBJECTS = np.array([[-0.22, 0.0, 0.3], [0.22, 0.0, 0.0], [0.6, -0.75 + 0.076, 0.25]])      # (x, y, theta), metres
CONSTANTS_OVEL = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [5.0, -6.0, 1.0]], np.float32)          # (ovx, ovy, ow), world units


def _C(kernel, name, constants, acts, toi):
    k = CONSTANT_KERNELS[kernel]
    cell, gw, gh = grid(scenes.W, scenes.H, R_DEFAULT)
    g = SimpleNamespace(name='%s-%s-toi%d' % (kernel, name, toi), kernel=kernel, constant=name, toi=toi, W=scenes.W, H=scenes.H, r=R_DEFAULT,
                        N=k['N'], sleep=0, family=k['family'], cell=cell, gw=gw, gh=gh, pitch=PITCH, acts=acts,
                        constants=dict(constants, toi_walls=toi), shapes=[], objects=None, ovel=None, mode_density=[2.0, 2.0, 0.0, 0.0, 0.0])
    if g.family == 'objects':
        g.shapes, g.objects, g.ovel = CONSTANTS_SHAPES, CONSTANTS_OBJECTS, CONSTANTS_OVEL
    return g


CONSTANTS = []
for _toi in (0, 1):
    for _kernel in CONSTANT_KERNELS:
        _rows = [('default', {}, None)] + BOT_CONSTANTS + (OBJ_CONSTANTS if _kernel == 'objects' else [])
        _rows.append(('all', dict(ALL_BOT, **(ALL_OBJ if _kernel == 'objects' else {})), 'bots'))
        CONSTANTS += [_C(_kernel, _n, _c, _a, _toi) for _n, _c, _a in _rows]


def control_of(g):
    """The row of default constants on the same scene and toi_walls."""
    return next(c for c in CONSTANTS if c.kernel == g.kernel and c.toi == g.toi and c.constant == 'default')
