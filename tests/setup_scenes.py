"""Scenes for the register set-up of the solver in the kernels without objects (kb_regsolve_bins.inc: light load, depth pass,
dealing, full load; kb_step_kernel.h: the grouping of the contacts by wave in front of it).

The set-up computes nothing but an ordering: which wave holds a contact, in which lane and slot, and in which round of a
sweep it runs.  A scene is built around one thing that ordering can get wrong:

    dealt           512 < contacts <= 688 on the eight waves of the fixed-size kernel: waves of more than 64 contacts, so the
                    dealing runs and both register slots are in use
    single slot     <= 512 contacts: no wave deals, slot 1 is empty in most waves
    wave counts     waves of exactly 64, of exactly 65 and of exactly 128 contacts (one env each, at the first launch)
    deep            a hexagonal cluster whose middle kilobot touches twelve others -- the contacts of one body all lie on
                    different depth levels, so its island is at least twelve levels deep -- next to hundreds of pairs (depth 1)
    rank bucket     the same cluster at the first launch, before it bursts: broadphase cells with five and more contacts in one
                    (cell, direction) group, i.e. ranks >= RK - 1, the open-ended bucket whose rounds go rank by rank (the
                    block of 'wave counts' keeps groups of four, rank RK - 1, through all its launches)
    walls           kilobots resting on a wall and one in a corner: A is a wall, two walls on one body
    normals         a pair with coincident centres (the normal stays (1, 0)), a pair 2^-22 world units apart (outside
                    kb_exact_guard: its wave takes the IEEE square root and division), ordinary pairs around them
    sleepers        (sleep instantiations) a block of kilobots asleep beside awake ones: key 63, depth 0, impulse carried over

Every env is made of motifs on a loose grid -- pairs and rows of three kilobots 32 mm apart (1 mm of overlap), single kilobots
-- plus the planted structure of the scene in a strip along the lower wall.  All of them must stay on the register path: no
island above GIANT_ISLAND contacts and no wave above 64 * KB_KREG_BINS.  Neither the wave of a contact, nor its rank, nor its
depth shows in what the oracle returns, so the rules are restated here from the kernel source:

    wave_loads      kb_step_kernel.h, "Placement of the islands on the waves in order of size" (BINS: the sweeping waves share
                    the contacts evenly, the largest islands first)
    rank groups     kb_step_kernel.h, stage_pass / label pass: the rank of a contact counts the contacts of its (base cell,
                    direction) group in front of it, so a group of g contacts has the ranks 0 .. g - 1
    depth           contacts that share a body lie on different levels: the busiest body's contacts bound the depth from below

Shared by tests/test_setup_pass_cpu.py (every scene has its property on the oracle) and tests/test_setup_pass_gpu.py (every
launch bit for bit against the oracle)."""
import functools
from types import SimpleNamespace

import numpy as np

from tests import label_scenes as LS
from tests import scenes
from tests.scenes import case_id, scene_id  # noqa: F401

LANES, KREG_BINS, GIANT_ISLAND, RK = 64, 2, 256, 4      # kb_common.h, kb_launch.h
WAVE_CONTACTS = LANES * KREG_BINS
WORLD = 25.0                    # world units per metre (kb_common.h: WORLD_SCALE)
LINK = 0.032                    # centre distance inside a motif (kilobot diameter 33 mm)
ROW_PITCH = 0.045
MOTIF_Y0, MOTIF_ROWS = -0.40, 25            # motif rows y = -0.40 .. 0.68
STRIP_Y = -0.70 + ROW_PITCH * np.arange(6)  # the strip of the planted structures and the spare single kilobots
SPACING = 0.019                 # of the hexagonal cluster (tests/label_scenes.py): first and second neighbours overlap
CLUSTER_RINGS = 2               # 19 kilobots, the middle one touches 12
DEEP = 12
BLOCK, TAIL = 8, 16             # an 8 x 8 block of touching kilobots (112 contacts) with a row of 16 more on one corner: 128
WALL_BOTS = 6
TINY = 2.0 ** -22               # world units between the two kilobots of the pair outside kb_exact_guard (dd = 2^-44 < 2^-40)
SLEEP_BLOCK = 4                 # 4 x 4 kilobots asleep: 24 contacts
SINGLE_LAUNCHES, FUSED_SUBSTEPS = 12, 10
SPEED = 0.03                    # of the commanded linear velocity

_E = lambda triples, pairs, *structs: SimpleNamespace(triples=triples, pairs=pairs, structs=structs)      # noqa: E731
_S = lambda name, N, envs, has, band=None, sleep_only=False: SimpleNamespace(                              # noqa: E731
    name=name, N=N, envs=envs, has=has, band=band, sleep_only=sleep_only)
# band: contacts of every env in every single-substep launch (inclusive)
SCENES = [
    _S('dealt-1024', 1024, [_E(200, 200), _E(190, 215)], ('dealt',), band=(513, 688)),
    _S('single-slot-1024', 1024, [_E(0, 400), _E(20, 330)], ('single slot',), band=(256, 512)),
    _S('wave-counts-1024', 1024, [_E(0, 512), _E(20, 480), _E(0, 440, 'block')], ('wave counts',), band=(400, 688)),
    _S('cluster-1024', 1024, [_E(190, 160, 'cluster'), _E(180, 170, 'cluster')], ('deep', 'rank bucket', 'dealt'), band=(513, 688)),
    _S('walls-1024', 1024, [_E(120, 300, 'walls'), _E(130, 290, 'walls')], ('walls', 'dealt'), band=(513, 688)),
    _S('normals-1024', 1024, [_E(100, 300, 'normals'), _E(0, 400, 'normals')], ('normals',), band=(300, 688)),
    _S('sleepers-1024', 1024, [_E(120, 280, 'sleepers'), _E(0, 380, 'sleepers')], ('sleepers',), band=(300, 688), sleep_only=True),
    # the generic sorted-bin kernel, two waves (N = 200: 128 threads): everything at once, <= 128 contacts per wave
    _S('mixed-200', 200, [_E(15, 60, 'cluster', 'walls', 'normals'), _E(13, 63, 'cluster', 'walls', 'normals')],
       ('deep', 'rank bucket', 'walls', 'normals', 'dealt'), band=(129, 256)),
    _S('sleepers-200', 200, [_E(10, 40, 'sleepers', 'walls'), _E(0, 50, 'sleepers', 'walls')], ('sleepers', 'walls'), band=(60, 256), sleep_only=True),
]
WAVE_COUNTS_FIRST = [[64] * 8, [65] * 8, [128, 14, 71, 71, 71, 71, 71, 71]]      # 'wave-counts-1024', contacts per wave at launch 0


cases = functools.partial(scenes.sleep_cases, SCENES)      # (scene, allow_sleep) of both test files


# ---- planted structures (metres) -----------------------------------------------------------------------------------------
def structure(kind):
    """[n, 2] around the origin of the structure (its lower left kilobot or its middle)"""
    if kind == 'cluster':
        return LS.hexagon(CLUSTER_RINGS) * SPACING + np.array([0.06, 0.06])
    if kind == 'block':
        i = np.arange(BLOCK * BLOCK)
        block = np.stack([i % BLOCK, i // BLOCK], -1) * 0.0325
        tail = np.stack([(BLOCK - 1) * 0.0325 + LINK * (1 + np.arange(TAIL)), np.zeros(TAIL)], -1)
        return np.concatenate([block, tail])
    if kind == 'sleepers':
        i = np.arange(SLEEP_BLOCK * SLEEP_BLOCK)
        return np.stack([i % SLEEP_BLOCK, i // SLEEP_BLOCK], -1) * 0.0325
    raise KeyError(kind)


def walls_xy():
    """kilobots 1.5 mm inside the lower wall's skin (40 mm apart), the last one in the lower left corner"""
    w = np.stack([-0.80 + 0.04 * np.arange(WALL_BOTS), np.full(WALL_BOTS, -0.75 + 0.015)], -1)
    w[-1] = (-1.0 + 0.015, -0.75 + 0.015)
    return w


def normals_xy():
    """[4, 2]: the coincident pair, then the pair TINY world units apart (both near the origin of the world frame, where a
    float has the digits for it)"""
    return np.array([[0.2, -0.5], [0.2, -0.5], [0.01, -0.5], [0.01 + TINY / WORLD, -0.5]])


def plant_env(N, env, rng):
    """(xy [N, 2] metres, asleep [N] bool, ids of the planted structures {kind: ids})"""
    xlim, rows = (0.95, MOTIF_ROWS) if N == 1024 else (0.5, 14)
    cur = [-xlim, 0]

    def slot(width):
        """middle of the next free stretch of `width` metres in the motif rows"""
        if cur[0] + width > xlim:
            cur[0], cur[1] = -xlim, cur[1] + 1
        assert cur[1] < rows, 'the motif rows are full'
        cur[0] += width
        return cur[0] - 0.5 * width, MOTIF_Y0 + ROW_PITCH * cur[1]
    pts, asleep, where = [], [], {}
    x0 = -0.60
    for kind in env.structs:
        if kind == 'walls':
            st = walls_xy()
        elif kind == 'normals':
            st = normals_xy()
        else:
            st = structure(kind) + np.array([x0, STRIP_Y[0]])
            x0 += st[:, 0].max() - st[:, 0].min() + 0.10
        where[kind] = np.arange(len(pts), len(pts) + len(st))
        pts += [tuple(p_) for p_ in st]
        asleep += [kind == 'sleepers'] * len(st)
    planted = np.array(pts).reshape(-1, 2)
    for n, count in ((3, env.triples), (2, env.pairs)):
        for _ in range(count):
            cx, cy = slot(0.11 if n == 3 else 0.075)
            pts += [(cx + LINK * (i - 0.5 * (n - 1)), cy) for i in range(n)]
    singles = N - len(pts)
    assert singles >= 0, 'too many kilobots planted: %d of %d' % (len(pts), N)
    spare = [(x, y) for y in STRIP_Y for x in -0.9 + ROW_PITCH * np.arange(41)]
    if len(planted):
        spare = [q for q in spare if (np.hypot(planted[:, 0] - q[0], planted[:, 1] - q[1]) > 0.07).all()]
    pts += spare[:singles]
    pts += [slot(0.05) for _ in range(singles - len(spare))]
    asleep += [False] * (len(pts) - len(asleep))
    perm = rng.permutation(N)           # ids in no relation to places: the id order (packed list) and the slot order differ
    xy = np.zeros((N, 2))
    xy[perm] = np.array(pts)
    sl = np.zeros(N, bool)
    sl[perm] = np.array(asleep)
    return xy, sl, {k: perm[v] for k, v in where.items()}


def plant(s):
    """(xy [E, N, 2] metres, theta [E, N], sleep_time [E, N] (-1: asleep), per env {kind: ids}); the motifs get 0.2 mm of
    jitter, the planted structures none"""
    rng = np.random.RandomState(5000 + s.N + 7 * len(s.name))
    E = len(s.envs)
    xy, st, ids = np.zeros((E, s.N, 2)), np.zeros((E, s.N), np.float32), []
    for e, env in enumerate(s.envs):
        xy[e], asleep, where = plant_env(s.N, env, rng)
        jit = rng.uniform(-0.0002, 0.0002, size=(s.N, 2))
        fixed = np.zeros(s.N, bool)
        for v in where.values():
            fixed[v] = True
        xy[e] += np.where(fixed[:, None], 0.0, jit)
        st[e, asleep] = -1.0
        ids.append(where)
    th = rng.uniform(-np.pi, np.pi, size=(E, s.N))
    return xy, th, st, ids


def actions(s, k, sleep_time):
    """fresh commands for launch k, U([0, 0.01] x [-pi/2, pi/2]) with SPEED of the speed -- the motifs press on each other
    and drift without coming apart inside the launches of a test; the sleepers are never commanded"""
    a = scenes.random_actions(len(s.envs), s.N, seed=900 + 20 * len(s.name) + k)
    a[..., 0] *= SPEED
    a[sleep_time < 0] = 0.0
    return a


# ---- what a substep has, from the oracle's packed list and the poses it started from -------------------------------------
def contacts(ws_key, ws_cnt):
    """(owner [n], key [n]) of one env's packed list"""
    return LS.lists(ws_key, ws_cnt)


def islands(ws_key, ws_cnt):
    """contacts per island of one env (wall contacts belong to their kilobot's island), largest first"""
    N = len(ws_cnt)
    parent = list(range(N))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    owner, key = contacts(ws_key, ws_cnt)
    for a, b in zip(owner, key):
        if b < LS.WALL_KEY:
            parent[find(int(a))] = find(int(b))
    size = np.bincount([find(int(a)) for a in owner], minlength=N)
    return sorted((int(n) for n in size if n), reverse=True)


def wave_loads(sizes, nsolve):
    """contacts per sweeping wave: the islands in order of size class (32 contacts and more are one class) take consecutive
    stretches of ceil(ncon / nsolve) contacts, an island goes to the wave its first contact falls on.  The order inside the
    class of 32 and more is not fixed: the answer is exact with at most one such island."""
    ncon = sum(sizes)
    chunk = max((ncon + nsolve - 1) // nsolve, 1)
    loads, at = [0] * nsolve, 0
    for n in sorted(sizes, reverse=True):
        loads[min(at // chunk, nsolve - 1)] += n
        at += n
    return loads


def on_register_path(sizes, nsolve):
    return bool(sizes) and sizes[0] <= GIANT_ISLAND and max(wave_loads(sizes, nsolve)) <= WAVE_CONTACTS


def cell_of(xy_m):
    c = np.floor((np.asarray(xy_m, np.float64) - [LS.XMIN, LS.YMIN]) / LS.CELL).astype(np.int64)
    return np.clip(c, 0, [LS.GW - 1, LS.GH - 1])


def largest_rank_group(ws_key, ws_cnt, xy_before_m):
    """contacts of the largest (base cell, direction) group among the kilobot - kilobot contacts of one env: the base cell is
    the owner's, the direction leads to the partner's cell"""
    owner, key = contacts(ws_key, ws_cnt)
    cell = cell_of(xy_before_m)
    groups = {}
    for a, b in zip(owner, key):
        if b < LS.WALL_KEY:
            g = tuple(sorted((tuple(cell[a]), tuple(cell[b]))))      # (the two cells name the group whichever end owns it)
            groups[g] = groups.get(g, 0) + 1
    return max(groups.values()) if groups else 0


def busiest_body(ws_key, ws_cnt):
    """contacts of the kilobot with the most contacts (walls included)"""
    owner, key = contacts(ws_key, ws_cnt)
    deg = np.bincount(owner, minlength=len(ws_cnt))
    deg += np.bincount(key[key < LS.WALL_KEY], minlength=len(ws_cnt))
    return int(deg.max())


def wall_contacts_of(ws_key, ws_cnt):
    """{kilobot: walls it touches}"""
    out = {}
    for a, b in LS.wall_contacts(ws_key, ws_cnt):
        out.setdefault(a, set()).add(b)
    return out
