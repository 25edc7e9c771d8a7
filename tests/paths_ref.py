"""Restatement of kb_sense_paths' definition (include/kilobots_hip.h), shared by the path tests.

The cell rule and the cell centres come from tests/grid_ref.py.  The blocked predicate restates the fixture walk of
kb_sense_objects on the tables of tests/objects_ref.py in float32, every operation its own float32 expression (the inside
flag and the squared distance of the winning candidate; objects_ref.restate_env returns the root of the latter only).  The
distances come from Dijkstra's algorithm with heapq on Python ints: deliberately not a sweep, so the restatement and the
kernel share no algorithm.  next, the kilobot rows and the stats follow the header word for word.  Comparisons with the
device are by equality of the bit patterns."""
import collections
import heapq

import numpy as np

from tests import grid_ref
from tests import objects_ref

f32 = np.float32
DIRS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))
NONE = -1       # D of a cell without a path, and of a blocked cell
Paths = collections.namedtuple('Paths', ('dist', 'step', 'bots', 'stats'))
PARTS = Paths._fields
bits = objects_ref.bits


def quant(length):
    """(int32) rint(min(max(l * 1024.0f, 1.0f), 65536.0f)) of a float32 length."""
    assert isinstance(length, np.float32)
    t = length * f32(1024.0)
    assert t.dtype == np.float32
    return int(np.rint(min(max(t, f32(1.0)), f32(65536.0))))


def costs(tab, gw, gh):
    """((qx, qy, qd), (udx, udy)): the integer step costs and the float32 unit vector of the diagonals."""
    _, _, cw, ch, _, _ = grid_ref.constants(tab, gw, gh)
    dg = np.sqrt(cw * cw + ch * ch)
    assert dg.dtype == np.float32
    return (quant(cw), quant(ch), quant(dg)), (cw / dg, ch / dg)


def weights(q):
    qx, qy, qd = q
    return [qd if k & 1 else qy if k & 2 else qx for k in range(8)]


def object_walk(tab, m, px_w, py_w, ox, oy, oth):
    """(inside [P] bool, best d2 [P] float32) of object m for points px_w, py_w [P] float32 (world units): the fixture walk
    of kb_sense_objects in float32."""
    so, co = objects_ref.sincos(np.array([oth], dtype=f32), f32)
    so, co = so[0], co[0]
    dx, dy = px_w - f32(ox), py_w - f32(oy)
    px, py = co * dx + so * dy, co * dy - so * dx
    P = px.shape[0]
    best, inside = np.full(P, np.inf, dtype=f32), np.zeros(P, dtype=bool)
    with np.errstate(divide='ignore', invalid='ignore'):
        for fx in tab['fixtures']:
            if fx['body'] != m:
                continue
            if fx['n'] == 0:
                g = np.sqrt(px * px + py * py) - fx['radius']
                d2 = g * g
                best = np.where(d2 < best, d2, best)
                inside |= ~(g > 0)
                continue
            v, in_f = fx['verts'], np.ones(P, dtype=bool)
            for k in range(fx['n']):
                a, b = v[k], v[(k + 1) % fx['n']]
                ex, ey = b[0] - a[0], b[1] - a[1]
                wx, wy = px - a[0], py - a[1]
                t = (wx * ex + wy * ey) / (ex * ex + ey * ey)
                clo, chi = ~(t > 0), t >= 1
                qx = np.where(clo, a[0], np.where(chi, b[0], a[0] + t * ex))
                qy = np.where(clo, a[1], np.where(chi, b[1], a[1] + t * ey))
                rx, ry = qx - px, qy - py
                d2 = rx * rx + ry * ry
                best = np.where(d2 < best, d2, best)
                in_f &= ex * wy - ey * wx >= 0
            inside |= in_f
    assert best.dtype == np.float32
    return inside, best


def object_block(tab, gw, gh, objects, clear_m, ox, oy, oth):
    """[gh, gw] bool: the object part of the blocked plane of one env."""
    cx, cy = grid_ref.centres(tab, gw, gh)
    blk = np.zeros(gw * gh, dtype=bool)
    cw_ = f32(clear_m) * f32(25.0)
    c2 = cw_ * cw_
    for m in range(tab['M']):
        if not objects >> m & 1:
            continue
        inside, d2 = object_walk(tab, m, cx, cy, ox[m], oy[m], oth[m])
        blk |= inside
        if clear_m > 0:
            blk |= ~(d2 > c2)
    return blk.reshape(gh, gw)


def allowed(free, ax, ay, k, corner=True):
    """Whether the move from the free cell (ax, ay) in direction k is allowed; free [gh, gw] bool."""
    gh, gw = free.shape
    dx, dy = DIRS[k]
    bx, by = ax + dx, ay + dy
    if not (0 <= bx < gw and 0 <= by < gh and free[by, bx]):
        return False
    return not (corner and k & 1) or bool(free[ay, bx] and free[by, ax])


def dijkstra(free, source, q, corner=True):
    """D [gh, gw] int64, summed as Python ints: the least sum of step costs from any free source cell along allowed moves
    (corner=False: without the corner rule), NONE where there is no path or the cell is blocked."""
    gh, gw = free.shape
    w = weights(q)
    D = [[NONE] * gw for _ in range(gh)]
    heap = [(0, int(iy), int(ix)) for iy, ix in np.argwhere(source & free)]
    done = np.zeros((gh, gw), dtype=bool)
    while heap:
        d, ay, ax = heapq.heappop(heap)
        if done[ay, ax]:
            continue
        done[ay, ax] = True
        D[ay][ax] = d
        for k in range(8):
            if allowed(free, ax, ay, k, corner):
                bx, by = ax + DIRS[k][0], ay + DIRS[k][1]
                if not done[by, bx]:
                    heapq.heappush(heap, (d + w[k], by, bx))
    D = np.array(D, dtype=np.int64).reshape(gh, gw)
    assert D.max(initial=0) < 2 ** 30
    return D


def descent(D, free, q, ax, ay, corner=True):
    """(least D(b) + w_k, lowest k attaining it) over the directions of (ax, ay) whose neighbour is inside the grid, free and
    reached (with corner: whose move is allowed); (NONE, -1) without one."""
    w, best, kb = weights(q), NONE, -1
    gh, gw = free.shape
    for k in range(8):
        bx, by = ax + DIRS[k][0], ay + DIRS[k][1]
        if not (0 <= bx < gw and 0 <= by < gh and free[by, bx] and D[by, bx] != NONE):
            continue
        if corner and not allowed(free, ax, ay, k):
            continue
        v = int(D[by, bx]) + w[k]
        if best == NONE or v < best:
            best, kb = v, k
    return best, kb


def metres(D):
    """((float)D / 1024.0f) / 25.0f of integers."""
    out = (np.asarray(D, dtype=np.int64).astype(np.float32) / f32(1024.0)) / f32(25.0)
    assert out.dtype == np.float32
    return out


def next_plane(D, free, source, q):
    gh, gw = free.shape
    nxt = np.full((gh, gw), -3, dtype=np.int8)
    for ay in range(gh):
        for ax in range(gw):
            if not free[ay, ax]:
                continue
            if D[ay, ax] == NONE:
                nxt[ay, ax] = -2
            elif source[ay, ax]:
                nxt[ay, ax] = -1
            else:
                v, k = descent(D, free, q, ax, ay)
                assert v == D[ay, ax], (ax, ay, v, D[ay, ax])
                nxt[ay, ax] = k
    return nxt


def restate_env(tab, gw, gh, source, blocked, objects, clear_m, x, y, th, ox=None, oy=None, oth=None):
    """One env: source, blocked [gh, gw] (blocked may be None), x, y, th [N], ox, oy, oth [M] float32 (world units, radians).
    Returns (Paths of numpy arrays, aux = {'D', 'free', 'src', 'flag'})."""
    q, (udx, udy) = costs(tab, gw, gh)
    blk = np.zeros((gh, gw), dtype=bool) if blocked is None else np.asarray(blocked) != 0
    if objects:
        blk = blk | object_block(tab, gw, gh, objects, clear_m, ox, oy, oth)
    free = ~blk
    src = (np.asarray(source) != 0) & free
    D = dijkstra(free, src, q)
    reached = D != NONE
    dist = np.where(reached, metres(np.where(reached, D, 0)), f32(np.inf)).astype(np.float32)
    step = next_plane(D, free, src, q)
    N = x.shape[0]
    ix, iy = grid_ref.cells(tab, gw, gh, x, y)
    sn, cs = objects_ref.sincos(th, f32)
    bots = np.zeros((N, 4), dtype=np.float32)
    flag = np.zeros(N, dtype=int)
    total, far, count = 0, 0, 0
    for i in range(N):
        ax, ay = int(ix[i]), int(iy[i])
        Db, kb = NONE, -1
        if free[ay, ax] and reached[ay, ax]:
            Db, kb, flag[i] = int(D[ay, ax]), int(step[ay, ax]), 1 if src[ay, ax] else 0
        elif not free[ay, ax]:
            Db, kb = descent(D, free, q, ax, ay, corner=False)
            flag[i] = 2 if Db != NONE else 3
        else:
            flag[i] = 3
        if Db == NONE:
            bots[i] = (np.inf, 0.0, 0.0, 3.0)
            continue
        count, total, far = count + 1, total + Db, max(far, Db)
        fx = fy = f32(0.0)
        if kb >= 0:
            dx, dy = DIRS[kb]
            ux, uy = f32(dx) * (udx if kb & 1 else f32(1.0)), f32(dy) * (udy if kb & 1 else f32(1.0))
            fx, fy = cs[i] * ux + sn[i] * uy, cs[i] * uy - sn[i] * ux
            assert fx.dtype == fy.dtype == np.float32
        bots[i] = (metres(Db), fx, fy, f32(flag[i]))
    stats = np.array([f32(count), metres(total), metres(far), f32(int(reached.sum()))], dtype=np.float32)
    return Paths(dist, step, bots, stats), dict(D=D, free=free, src=src, flag=flag, q=q)


def restate(tab, gw, gh, source, blocked, objects, clear_m, x, y, th, ox=None, oy=None, oth=None):
    """source, blocked [E, gh, gw] (blocked may be None), x, y, th [E, N], ox, oy, oth [E, M] or None -> (Paths of stacked
    arrays, [aux per env])."""
    E = x.shape[0]
    none = [None] * E
    blocked = none if blocked is None else blocked
    ox, oy, oth = (none if v is None else v for v in (ox, oy, oth))
    envs = [restate_env(tab, gw, gh, source[e], blocked[e], objects, clear_m, x[e], y[e], th[e], ox[e], oy[e], oth[e]) for e in range(E)]
    return Paths(*(np.stack([getattr(p, n) for p, _ in envs]) for n in PARTS)), [a for _, a in envs]


# ---- the scenes of the tests: cell masks -----------------------------------------------------------------------------------
def serpentine(gw, gh):
    """blocked [gh, gw] uint8: every other row is a wall with a one-cell gap at alternating ends, so that the free cells form
    one corridor from (0, 0) through every even row: the worst case for the sweep count."""
    blk = np.zeros((gh, gw), dtype=np.uint8)
    for n, iy in enumerate(range(1, gh, 2)):
        blk[iy, :] = 1
        blk[iy, gw - 1 if n % 2 == 0 else 0] = 0
    return blk


def corner_scene(gw=7, gh=5):
    """blocked [gh, gw] uint8: two obstacles that touch at a corner and together cut the grid in two but for the top row:
    without the corner rule the short way to the far side is the diagonal squeeze between them, with it the detour through
    the top row."""
    blk = np.zeros((gh, gw), dtype=np.uint8)
    cx = gw // 2
    blk[:gh // 2, cx] = 1               # the lower obstacle: column cx up to the middle row (exclusive)
    blk[gh // 2:gh - 1, cx - 1] = 1     # the upper one: column cx - 1 from the middle row, touching the lower at a corner
    return blk


def mask_of(gw, gh, cells):
    m = np.zeros((gh, gw), dtype=np.uint8)
    for ix, iy in cells:
        m[iy, ix] = 1
    return m


def cell_centre_m(gw, gh, ix, iy, world=(2.0, 1.5)):
    """The centre of cell (ix, iy) of a gw x gh grid over an arena of `world` metres about the origin, in metres (float64:
    for placing kilobots well inside a cell, not for comparing)."""
    return (-world[0] / 2 + (ix + 0.5) * world[0] / gw, -world[1] / 2 + (iy + 0.5) * world[1] / gh)


def mixed_scene():
    """(gw, gh, source, blocked [gh, gw] uint8, xy [N, 2] metres, th [N]) on the default 2 x 1.5 m arena: 7 x 5 non-square
    cells; columns 4 and 5 are walls, so column 6 is free and cut off; three sources, two of them two cells apart (the cell
    between them and the one above it have tied directions).  The kilobots: on a source, on a free reached cell, on the wall
    with a way out (column 4), on the wall without one (column 5), on a free cell that is cut off, and two outside the
    arena, whose cells clamp to a reached edge cell and to the cut-off corner."""
    gw, gh = 7, 5
    blocked = np.zeros((gh, gw), dtype=np.uint8)
    blocked[:, 4:6] = 1
    source = mask_of(gw, gh, [(0, 0), (2, 0), (1, 3), (5, 2)])      # (the last one is blocked: no source)
    cells = [(0, 0), (2, 2), (4, 2), (5, 1), (6, 4)]
    xy = [cell_centre_m(gw, gh, ix, iy) for ix, iy in cells] + [(-1.5, 0.1), (3.0, 3.0)]
    th = np.random.RandomState(11).uniform(-np.pi, np.pi, size=len(xy))
    return gw, gh, source, blocked, np.array(xy), th


def scattered(E, N, seed):
    """Kilobots all over the default arena and a little beyond it (their cells clamp), random headings."""
    rng = np.random.RandomState(seed)
    return rng.uniform(-1.0, 1.0, size=(E, N, 2)) * [1.15, 0.85], rng.uniform(-np.pi, np.pi, size=(E, N))


def random_masks(E, gw, gh, seed, density=0.25, sources=3):
    """(source, blocked) [E, gh, gw] uint8: blocked cells at random, a few sources (some of them on blocked cells)."""
    rng = np.random.RandomState(seed)
    blocked = (rng.rand(E, gh, gw) < density).astype(np.uint8)
    source = np.zeros((E, gh, gw), dtype=np.uint8)
    for e in range(E):
        source[e].reshape(-1)[rng.randint(0, gw * gh, size=sources)] = 1
        if not (source[e] & (1 - blocked[e])).any():        # at least one free source
            blocked[e].reshape(-1)[np.flatnonzero(source[e])[0]] = 0
    return source, blocked
