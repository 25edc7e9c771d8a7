"""tools/box2d_mini.py against itself: the general b2TimeOfImpact (b2Distance with its simplex cache, b2SeparationFunction
with its three types, push-back loop, bisection / secant root finder) against the closed-form edge-circle routine that the
kilobot and disc scenes have used since the first fixture.  This validates the GJK and root-finder code on pairs where a
second answer exists, before anything is concluded from it about polygons (tests/test_oracle_vs_mini_solver.py).

Both routines must name the same state.  Where that state is `touching`, the distance between the circle's centre and the
edge at the general routine's t -- evaluated in float64, independently of either routine -- must lie within Box2D's own
band, target +- tolerance = max(slop, r_edge + r_circle - 3 slop) +- slop / 4.  Nothing here is measured.

A sweep that STARTS below the band (deeper than target - tolerance without overlapping) is answered `touching, t = 0` by
Box2D's first exit, outside the band by construction, so no family starts there.

An edge and a circle, and a polygon inside the arena, only ever reach `e_faceA` (and `e_points` at an edge's end), and never
a 3-simplex.  The last tests therefore run pairs of boxes: known distances from b2Distance (face to face, vertex to face,
corner to corner, overlap through b2Simplex::Solve3) and b2TimeOfImpact through each of the three separation-function types,
checked against a float64 vertex-to-segment distance written here."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import box2d_mini as B  # noqa: E402

R = 0.4125                                   # a kilobot
SLOP, POLY_R = 0.005, 0.01
TARGET = max(SLOP, POLY_R + R - 3.0 * SLOP)
TOL = 0.25 * SLOP
X1, X2 = -2.0, 2.0                           # the edge lies on the x axis


def _sweeps():
    """[(family, c0, c1, a0, a1, circle offset)] : about 50 seeded sweeps of the body's centre of mass"""
    rng = np.random.default_rng(20231)
    out = []
    for k in range(16):                      # head-on: from well above the edge to inside or beyond it, from either side
        side = 1.0 if k % 4 else -1.0
        x = rng.uniform(-1.5, 1.5)
        out.append(('head_on', (x, side * rng.uniform(0.6, 2.0)), (x + rng.uniform(-0.5, 0.5), side * rng.uniform(-1.0, 0.3))))
    for k in range(12):                      # grazing: the sweep ends around the band, so `touching` and `separated` both occur
        x = rng.uniform(-1.5, 1.0)
        out.append(('grazing', (x, rng.uniform(0.5, 0.9)), (x + rng.uniform(0.2, 0.8), TARGET + rng.uniform(-3.0, 3.0) * TOL)))
    for k in range(8):                       # starting inside the target band
        x = rng.uniform(-1.5, 1.5)
        out.append(('in_band', (x, TARGET + rng.uniform(-0.9, 0.9) * TOL), (x + rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 1.0))))
    for k in range(8):                       # separated at t = 1: approaching, but not far enough (or leaving)
        x = rng.uniform(-1.5, 1.5)
        out.append(('separated', (x, rng.uniform(0.8, 2.0)), (x + rng.uniform(-0.5, 0.5), TARGET + rng.uniform(2.0, 200.0) * TOL)))
    for k in range(6):                       # aimed at the edge's end vertex (X2, 0) from beyond the end: the simplex is one point
        ang = rng.uniform(0.3, 1.2)
        d = (math.cos(ang), math.sin(ang))
        out.append(('end_vertex', (X2 + 1.5 * d[0], 1.5 * d[1]), (X2 - 0.2 * d[0], -0.2 * d[1])))
    sweeps = []
    for k, (family, c0, c1) in enumerate(out):
        # every other head-on and grazing sweep turns, with the circle off the body's centre of mass (a second fixture moves
        # that): the swept transform p = c - R localCenter then matters
        spin = k % 2 == 1 and family in ('head_on', 'grazing')
        a0 = float(rng.uniform(-7.0, 7.0)) if spin else 0.0
        sweeps.append((family, c0, c1, a0, a0 + (float(rng.uniform(-1.0, 1.0)) if spin else 0.0), (0.07, -0.04) if spin else (0.0, 0.0)))
    return sweeps


SWEEPS = _sweeps()


def _world(c0, c1, a0, a1, offset):
    w = B.World()
    table = w.create_body(dynamic=False)
    edge = table.create_fixture(B.Edge((X1, 0.0), (X2, 0.0)), density=0.0)
    body = w.create_body(position=c0, angle=a0)
    disc = body.create_fixture(B.Circle(R, B.V(*offset)), density=2.0)
    if offset != (0.0, 0.0):
        body.create_fixture(B.Circle(0.2, B.V(-0.3, 0.25)), density=2.0)
    # the sweep of b2Body: the centre of mass goes from c0 to c1, the angle from a0 to a1
    body.c0, body.c, body.a0, body.a = B.V(*c0), B.V(*c1), B.f32(a0), B.f32(a1)
    return table, edge, body, disc


def _centre64(body, disc, t):
    """the circle's centre at time t of the sweep, in float64"""
    c = (1.0 - t) * np.array(body.c0.tup()) + t * np.array(body.c.tup())
    a = (1.0 - t) * float(body.a0) + t * float(body.a)
    rel = np.array(disc.shape.p.tup()) - np.array(body.local_center.tup())
    return c + np.array([math.cos(a) * rel[0] - math.sin(a) * rel[1], math.sin(a) * rel[0] + math.cos(a) * rel[1]])


def _edge_distance64(p):
    x = min(max(p[0], X1), X2)
    return math.hypot(p[0] - x, p[1])


@pytest.mark.parametrize('k', range(len(SWEEPS)))
def test_general_time_of_impact_agrees_with_the_closed_form(k):
    family, c0, c1, a0, a1, offset = SWEEPS[k]
    assert B.precision() == 32
    table, edge, body, disc = _world(c0, c1, a0, a1, offset)
    state_c, t_c = B.time_of_impact_edge_circle(edge.shape, table, disc.shape, body)
    state_g, t_g = B.time_of_impact(B.DistanceProxy(edge.shape), B.Sweep.of(table), B.DistanceProxy(disc.shape), B.Sweep.of(body))
    d = _edge_distance64(_centre64(body, disc, float(t_g)))
    print(family, 'closed form', state_c, float(t_c), 'general', state_g, float(t_g), 'distance at t', d, 'band', TARGET - TOL, TARGET + TOL)
    assert state_g == state_c, (family, state_g, state_c)
    if family == 'separated':
        assert state_g == 'separated'
    if family in ('head_on', 'end_vertex', 'in_band'):
        assert state_g == 'touching'
    if state_g == 'touching':
        assert TARGET - TOL <= d <= TARGET + TOL, (family, d)
        if family == 'in_band':
            assert float(t_g) == 0.0


def test_families_see_both_outcomes():
    """the grazing family is only worth its name if it holds sweeps that touch and sweeps that stay separated"""
    states = set()
    for family, c0, c1, a0, a1, offset in SWEEPS:
        if family == 'grazing':
            table, edge, body, disc = _world(c0, c1, a0, a1, offset)
            states.add(B.time_of_impact(B.DistanceProxy(edge.shape), B.Sweep.of(table), B.DistanceProxy(disc.shape), B.Sweep.of(body))[0])
    assert states == {'touching', 'separated'}


# ---- polygon pairs: the simplex solvers and the two separation-function types that an edge-circle pair cannot reach
def _still(x, y, a=0.0):
    return B.Sweep(B.V(), B.V(x, y), a, B.V(x, y), a)


def _xf(x, y, a=0.0):
    return B.XF(B.V(x, y), B.Rot(a))


@pytest.mark.parametrize('bx,by,ba,want,count', [
    (3.0, 0.5, 0.0, 1.0, 2),                                  # face to face: a 2-simplex (the flat case ends on a degenerate one)
    (3.0, 0.0, math.pi / 4, 2.0 - math.sqrt(2.0), 2),         # vertex to face
    (3.0, 3.0, 0.0, math.sqrt(2.0), 1),                       # corner to corner: one point
    (1.5, 0.5, 0.3, 0.0, 3),                                  # overlap: the origin inside a 3-simplex (b2Simplex::Solve3)
])
def test_distance_known_answers_between_two_boxes(bx, by, ba, want, count):
    box = B.DistanceProxy(B.Polygon.box(1.0, 1.0))
    cache = B.SimplexCache()
    pA, pB, d, it = B.distance(cache, box, _xf(0.0, 0.0), box, _xf(bx, by, ba))
    assert abs(float(d) - want) <= 4e-7 * max(1.0, want) and cache.count == count and it <= 20, (float(d), cache.count, it)
    # warm-started from its own cache the answer is the same (parallel faces may move the witness points along the faces)
    _, _, d2, it2 = B.distance(cache, box, _xf(0.0, 0.0), box, _xf(bx, by, ba))
    assert abs(float(d2) - want) <= 4e-7 * max(1.0, want) and it2 <= 20 and cache.count == count


def _world_vertices64(sweep, t):
    """the unit box's vertices at time t of a sweep (local centre zero), in float64"""
    x = (1.0 - t) * float(sweep.c0.x) + t * float(sweep.c.x)
    y = (1.0 - t) * float(sweep.c0.y) + t * float(sweep.c.y)
    a = (1.0 - t) * float(sweep.a0) + t * float(sweep.a)
    return [(x + math.cos(a) * lx - math.sin(a) * ly, y + math.sin(a) * lx + math.cos(a) * ly) for lx, ly in ((-1, -1), (1, -1), (1, 1), (-1, 1))]


def _polygon_distance64(P, Q):
    """distance of two disjoint convex polygons: the smallest vertex-to-segment distance, both ways"""
    def seg(p, a, b):
        ex, ey = b[0] - a[0], b[1] - a[1]
        u = min(1.0, max(0.0, ((p[0] - a[0]) * ex + (p[1] - a[1]) * ey) / (ex * ex + ey * ey)))
        return math.hypot(p[0] - a[0] - u * ex, p[1] - a[1] - u * ey)
    return min(min(seg(p, Q[i], Q[(i + 1) % len(Q)]) for p in P for i in range(len(Q))),
               min(seg(q, P[i], P[(i + 1) % len(P)]) for q in Q for i in range(len(P))))


def _types_seen(run):
    seen, init = [], B.SeparationFunction.__init__

    def spy(self, *a):
        init(self, *a)
        seen.append(self.type)
    B.SeparationFunction.__init__ = spy
    try:
        out = run()
    finally:
        B.SeparationFunction.__init__ = init
    return out, seen


@pytest.mark.parametrize('case', ['faceB', 'faceA', 'points'])
def test_time_of_impact_of_two_polygons_known_answer(case):
    """A diamond (a unit box turned by 45 degrees, its vertex at x = sqrt 2) at rest and a unit box that flies at it.  faceB:
    the box comes face first (one point on A, two on B); faceA: the roles swapped; points: the box comes corner first at the
    diamond's vertex, turning.  The state is `touching`, and at the returned t the float64 distance of the two polygons
    lies in Box2D's band max(slop, 2 polygonRadius - 3 slop) +- slop / 4; the mover must have used the separation function
    the case is named after."""
    box = B.DistanceProxy(B.Polygon.box(1.0, 1.0))
    target, tol, rt2 = 0.005, 0.00125, math.sqrt(2.0)
    diamond = _still(0.0, 0.0, math.pi / 4)
    if case == 'points':
        mover = B.Sweep(B.V(), B.V(4.0, 0.0), math.pi / 4, B.V(2.0, 0.0), math.pi / 4 + 0.05)
    else:
        mover = B.Sweep(B.V(), B.V(5.0, 0.3), 0.0, B.V(1.0, 0.3), 0.0)
    args = (box, mover, box, diamond) if case == 'faceA' else (box, diamond, box, mover)
    (state, t), seen = _types_seen(lambda: B.time_of_impact(*args))
    assert state == 'touching' and case in seen, (state, seen)
    t = float(t)
    d = _polygon_distance64(_world_vertices64(args[1], t), _world_vertices64(args[3], t))
    print(case, 'types', seen, 't', t, 'distance', d, 'band', target - tol, target + tol)
    assert target - tol - 2e-6 <= d <= target + tol + 2e-6, (case, d)      # 2e-6: float32 rounding of coordinates of size 4
