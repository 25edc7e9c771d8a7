"""Scenes for the continuous step of the kilobots against the walls (kb_step_kernel.h, "continuous step"; kb_common.h:
kb_toi_wall, kb_toi_no_event, kb_toi_walls_body) and the restated rule by which the kernel decides who enters it.

The kernel takes a kilobot through the event loop only if kb_toi_no_event is false for some wall.  For one wall, with d0 and
d1 the wall distances of the centre at the start of the substep and behind the position sweeps and tt = target + tolerance of
b2TimeOfImpact,

    no event possible  <=>  |d0| <= 0  or  (not |d0| < tt  and  d1 > tt)

(no_event below, in numpy float32 with the kernel's expressions).  tests/test_toi_filter_cpu.py shows on the oracle that a
kilobot for which this holds on all four walls leaves the continuous step exactly as it came; tests/test_toi_filter_gpu.py
steps the same scenes on the device.

What is planted along the walls (world units; a kilobot at full speed covers `step` = 0.0231 per substep, tt = total - 0.01375):

    pressed     driven head-on into a wall from total - slop / 2, and into each corner: held by the contact, at rest for every
                substep.  Inside `total` (the reject that was there before lets them through), outside tt, never an event
    ram         head-on from total + 0.004 + m step: free for m substeps, then from outside `total` to inside tt in one: an event.
                Some land early, some inside the fused launch at the end (substeps 13, 15, 16, 17, 19), so that env 1, which has
                no permanent candidate, has env-substeps with and without a candidate among the single launches AND inside the
                fused one -- the kernels take the processing loop and its barriers in the former and go round them in the latter
    ram40/50    the same 40 and 50 degrees off the normal -- the shallowest angles at which the normal travel of one substep
                still bridges total - tt
    graze       75 degrees off the normal: slides into the contact skin over several substeps, never an event
    corner      along the diagonal from total + 0.001 off both walls: both walls fall in the same substep
    static      at rest with the centre ON the wall line (d0 == 0), beyond it (d0 < 0: a candidate in every substep; env 0 only), and with d0 one fp32 step inside tt,
                on tt and one step outside it, and on the two fp32 values around `total`
    timed       free runs at full speed whose END distance of the first substep lies one step inside tt, on tt, one step
                outside it, and on the two values around `total`: the start is found by bisection with the oracle
    sleepers    (sleep state) a 3 x 3 block asleep on the lower wall, inside `total`

In the default arena the wall-side coordinates lie in [16, 32), where fp32 has a spacing of GRID = 2^-19, and a wall distance is
an exact multiple of it; tt has six more digits.  The scenes of 16 and 200 kilobots therefore take the kilobot radius next to
the default one for which tt is a multiple of GRID (grid_radius: < 1e-6 m off), so that d0 == tt and d1 == tt exist; the scene
of 1024 kilobots has the default radius and the values on either side."""
import functools
from types import SimpleNamespace

import numpy as np

from tests.scenes import case_id  # noqa: F401

f32 = np.float32
WORLD = 25.0                                # world units per metre
WS, SLOP = f32(25.0), f32(0.005)
POLYGON_RADIUS = f32(2.0) * SLOP
XMIN, YMIN, XMAX, YMAX = f32(-25.0), f32(-18.75), f32(25.0), f32(18.75)     # default arena, 2 m x 1.5 m
GRID = 2.0 ** -19
FULL = 0.01                                 # m/s, the upper end of the action space
DEFAULT_RADIUS = 0.0165
SINGLE_LAUNCHES, FUSED_SUBSTEPS = 12, 10
SUBSTEPS = SINGLE_LAUNCHES + FUSED_SUBSTEPS
SLOT_PITCH = 1.5                            # along a wall, between planted kilobots (diameter 0.825)
STATIC = ('on-line', 'beyond', 'tt-1', 'tt', 'tt+1', 'total-', 'total+')
TIMED = ('end tt-1', 'end tt', 'end tt+1', 'end total-', 'end total+')
MOVING = ('pressed', 'ram', 'ram40', 'graze', 'ram', 'ram50', 'pressed', 'ram')
PHI = {'pressed': 0.0, 'ram': 0.0, 'ram40': np.radians(40.0), 'ram50': np.radians(50.0), 'graze': np.radians(75.0)}
CORNERS = ((0, 1), (2, 1), (2, 3), (0, 3))
LATE = (15, 19, 17)                         # substeps in which late rammers land: inside the fused launch, not in all of it
RAM_DELAYS = (0, 1, 2, 3, 5, 13, 16, 19)    # free substeps of the head-on rammers of the mixed scenes

_S = lambda name, N, radius, sleepers: SimpleNamespace(name=name, N=N, radius=radius, sleepers=sleepers)      # noqa: E731


def thresholds(radius):
    """(total, tt) in float32, by the operations of kb_toi_wall: total = R + polygonRadius,
    tt = fmaxf(slop, total - 3 slop) + 0.25 slop"""
    total = f32(radius) * WS + POLYGON_RADIUS
    tt = np.maximum(SLOP, total - f32(3.0) * SLOP) + f32(0.25) * SLOP
    assert total.dtype == np.float32 and tt.dtype == np.float32
    return total, tt


@functools.lru_cache(None)
def grid_radius():
    """the float32 radius (metres) next to the default one for which tt is a multiple of GRID"""
    r = f32(DEFAULT_RADIUS)
    for _ in range(1 << 12):
        q = float(thresholds(r)[1]) / GRID
        if q == round(q):
            return float(r)
        r = np.nextafter(r, f32(1.0))
    raise AssertionError('no radius with tt on the grid')


def scenes():
    return [_S('thresholds-16', 16, grid_radius(), False), _S('mixed-200', 200, grid_radius(), True),
            _S('mixed-1024', 1024, DEFAULT_RADIUS, True)]


def cases():
    """(scene, allow_sleep): the scene of 16 kilobots has no sleepers and runs without the sleep state only"""
    return [(s, sl) for s in scenes() for sl in (0, 1) if s.sleepers or not sl]


# ---- the rule, restated ----------------------------------------------------------------------------------------------------
def wall_dists(x, y):
    """[4, ...] float32: wall_geom's distances of a centre to the walls xmin, ymin, xmax, ymax"""
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    return np.stack([x - XMIN, y - YMIN, XMAX - x, YMAX - y])


def _lerp(t, a0, a1):
    return (f32(1.0) - f32(t)) * np.asarray(a0, f32) + f32(t) * np.asarray(a1, f32)


def sweep_dists(x0, y0, x1, y1):
    """(d0, d1), [4, ...] each: kb_toi_wall's dist_at(0) and dist_at(1) for every wall"""
    with np.errstate(invalid='ignore'):
        return wall_dists(_lerp(0.0, x0, x1), _lerp(0.0, y0, y1)), wall_dists(_lerp(1.0, x0, x1), _lerp(1.0, y0, y1))


def no_event(d0, d1, tt):
    """[4, ...] bool: the wall can have no event.  The negation is kept as written: an unordered compare keeps the candidate."""
    with np.errstate(invalid='ignore'):
        return (np.abs(d0) <= f32(0.0)) | (~(np.abs(d0) < tt) & (d1 > tt))


def old_reject_passes(x0, y0, x1, y1, total):
    """[...] bool: the quick reject on `total` alone (start or end within `total` of some wall) lets the kilobot through"""
    m0, m1 = wall_dists(x0, y0).min(0), wall_dists(x1, y1).min(0)
    return ~((m0 > total) & (m1 > total))


# ---- placement -------------------------------------------------------------------------------------------------------------
def at_wall(wl, d, s):
    """(x, y, heading into the wall) of a centre d off wall wl at s along it, world units in float64"""
    if wl == 0:
        return float(XMIN) + d, s, np.pi
    if wl == 1:
        return s, float(YMIN) + d, -0.5 * np.pi
    if wl == 2:
        return float(XMAX) - d, s, 0.0
    return s, float(YMAX) - d, 0.5 * np.pi


def free_end_dist(radius, wl, d, s, phi=0.0):
    """wall distance (float32) behind one substep WITHOUT the continuous step of a lone kilobot that starts d off wall wl at
    full speed, phi off the normal: the oracle's own arithmetic"""
    from oracle import oracle as O
    o = O.OracleSim(O.default_config(1, 1, O.DRIVE_VELOCITY, O.LIGHT_NONE, bot_radius=radius, toi_walls=0, allow_sleep=0))
    x, y, th = at_wall(wl, d, s)
    o.set_poses_m(np.array([[[x / WORLD, y / WORLD]]]), np.array([[th + phi]]))
    o.set_actions(np.array([[[FULL, 0.0]]], f32))
    o.step(1)
    return wall_dists(o.x[0, 0], o.y[0, 0])[wl]


@functools.lru_cache(None)
def step_length(radius):
    """world units a free kilobot covers in one substep at full speed"""
    return 5.0 - float(free_end_dist(radius, 0, 5.0, 0.0))


@functools.lru_cache(None)
def timed_start(radius, wl, s, target):
    """k: the largest start distance k * GRID, outside `total`, from which a head-on run at full speed ends its first substep
    at a wall distance <= target (bisection over k)"""
    total = float(thresholds(radius)[0])
    end = lambda k: float(free_end_dist(radius, wl, k * GRID, s))      # noqa: E731
    lo = int(np.ceil(total / GRID)) + 1
    hi = lo + int(0.05 / GRID)
    assert end(lo) <= target < end(hi), (end(lo), target, end(hi))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if end(mid) <= target:
            lo = mid
        else:
            hi = mid
    return lo


def _slots(wl):
    half = float(XMAX if wl in (1, 3) else YMAX)
    lo = -half + 8.5 if wl == 1 else -half + 2.5           # (the lower wall keeps its left end for the sleepers)
    return list(np.arange(lo, half - 2.4, SLOT_PITCH))


def plant_env(s, e, rng):
    """rows (x, y, theta, v, w, asleep) of env e, world units, and {kind: ids}"""
    total, tt = (float(v) for v in thresholds(s.radius))
    step = step_length(s.radius)
    rows, where = [], {}

    def add(kind, wl, d, sl, phi=0.0, v=FULL, asleep=False):
        x, y, th = at_wall(wl, d, sl)
        where.setdefault(kind, []).append(len(rows))
        rows.append((x, y, th + phi, v, 0.0, asleep))

    def planted(wl, sl):
        """the seven static and the five timed kilobots of the thresholds on wall wl, from slot list sl.  The kilobot beyond
        the wall line stays a candidate in every substep while it is awake: env 0 has it, env 1 a late rammer in its place"""
        below = lambda v: int(np.floor(v / GRID))      # noqa: E731
        k_tt, k_total = below(tt), below(total)
        for kind, d in zip(STATIC, (0.0, -0.1, (k_tt - 1) * GRID, k_tt * GRID, (k_tt + 1) * GRID, k_total * GRID, (k_total + 1) * GRID)):
            if kind == 'beyond' and e == 1:
                add('ram', wl, total + 0.004 + LATE[2] * step, sl.pop(0))
            else:
                add(kind, wl, d, sl.pop(0), v=0.0)
        for kind, target, dk in zip(TIMED, (tt, tt, tt, total, total), (-1, 0, 1, 0, 1)):
            at = sl.pop(0)
            add(kind, wl, (timed_start(s.radius, wl, at, target) + dk) * GRID, at)

    def corner(kind, c, d):
        (x, _, _), (_, y, _) = at_wall(c[0], d, 0.0), at_wall(c[1], d, 0.0)
        where.setdefault(kind, []).append(len(rows))
        rows.append((x, y, np.arctan2(-1.0 if c[1] == 1 else 1.0, -1.0 if c[0] == 0 else 1.0), FULL, 0.0, False))

    if s.N == 16:
        wl = (0, 3)[e]
        planted(wl, _slots(wl))
        others = [o for o in range(4) if o != wl]
        add('pressed', others[0], total - 0.5 * float(SLOP), 0.0)
        add('ram', others[1], total + 0.004 + 3 * step, 0.0)
        add('ram', others[2], total + 0.004 + LATE[0] * step, 0.0)
        corner('corner', CORNERS[e], total + 0.001)
    else:
        free = {wl: _slots(wl) for wl in range(4)}
        for wl in ((e, e + 2) if s.N == 200 else range(4)):
            planted(wl, free[wl])
        for wl in range(4):
            for i, sl in enumerate(free[wl]):
                kind = MOVING[(i + wl) % len(MOVING)]
                cosphi = np.cos(PHI[kind])
                d = {'pressed': total - 0.5 * float(SLOP), 'graze': total + 0.004, 'ram50': total + 0.0005 + (i % 3) * step * cosphi,
                     'ram40': total + 0.002 + (i % 4) * step * cosphi, 'ram': total + 0.004 + RAM_DELAYS[i % len(RAM_DELAYS)] * step}[kind]
                add(kind, wl, d, sl + rng.uniform(-0.05, 0.05), phi=PHI[kind] * (1 if wl % 2 else -1))      # (one sense per wall: neighbours keep their distance)
        for i, c in enumerate(CORNERS):
            corner(*(('corner', c, total + 0.001) if (i + e) % 2 else ('pressed corner', c, total - 0.5 * float(SLOP))))
        if s.sleepers:
            for i in range(9):
                add('sleepers', 1, total - 0.5 * float(SLOP) + 0.82 * (i // 3), float(XMIN) + 3.0 + 0.82 * (i % 3), v=0.0, asleep=True)
        # the rest: a lattice in the middle of the arena under random commands
        pitch = 1.05
        spots = [(x, y) for y in np.arange(-13.5, 13.6, pitch) for x in np.arange(-19.5, 19.6, pitch)]
        need = s.N - len(rows)
        assert 0 <= need <= len(spots), (need, len(spots))
        for i in rng.choice(len(spots), need, replace=False):
            where.setdefault('filler', []).append(len(rows))
            rows.append((spots[i][0], spots[i][1], rng.uniform(-np.pi, np.pi), rng.uniform(0.0, FULL), rng.uniform(-0.5 * np.pi, 0.5 * np.pi), False))
    assert len(rows) == s.N, (len(rows), s.N)
    return np.array(rows, np.float64), {k: np.array(v) for k, v in where.items()}


@functools.lru_cache(None)
def _plant(name):
    s = next(s_ for s_ in scenes() if s_.name == name)
    rng = np.random.RandomState(7100 + s.N)
    E = 2
    rows, ids = zip(*(plant_env(s, e, rng) for e in range(E)))
    rows = np.stack(rows)
    perm = np.stack([rng.permutation(s.N) for _ in range(E)])        # ids in no relation to places: `b` and `b + nt` of a thread lie anywhere
    out = np.zeros_like(rows)
    for e in range(E):
        out[e, perm[e]] = rows[e]
    return out, [{k: perm[e][v] for k, v in ids[e].items()} for e in range(E)]


def plant(s):
    """(xy [E, N, 2] metres, theta [E, N], actions [E, N, 2], sleep_time [E, N] (-1: asleep), per env {kind: ids})"""
    rows, ids = _plant(s.name)
    xy = rows[..., 0:2] / WORLD
    acts = rows[..., 3:5].astype(f32)
    st = np.where(rows[..., 5] > 0, -1.0, 0.0).astype(f32)
    return xy, rows[..., 2].copy(), acts, st, ids
