#!/usr/bin/env python3
"""Runs small scenes through the independent mini-solver (tools/box2d_mini.py) and writes their trajectories to
tests/golden/mini_solver.json.  tests/test_oracle_vs_mini_solver.py replays the same scenes on the oracle.

    python tools/gen_mini_solver_golden.py            # rewrite the fixture
    python tools/gen_mini_solver_golden.py --check    # regenerate in memory and compare with the committed fixture
Scene format (all lengths in Box2D world units = metres x 25, like the reference's b2Body values):
  kilobots: [[x, y, theta, v_cmd m/s, omega_cmd rad/s], ...]  SimpleVelocityControlKilobot (kilobot.py:213-263): every substep
            the env writes v = 25 v_cmd (cos theta, sin theta), omega = omega_cmd into the body, then world.Step
  objects:  [{shape: circle|box, r | hx, hy, x, y, theta, vx, vy, w}, ...]   density 2, friction 0.01, damping 0.8 (body.py:11-16)
            or by class: {shape: Triangle|LForm|TForm|CForm|polygon, width, height [m], (verts for polygon), x, y, ...}: the
            unit outline of gym_kilobots_amd/lib/body.py (`_shape_vertices()`), scaled and recentred as the reference's
            Polygon does (restated in `sub_polygons`), every convex part through b2PolygonShape::Set as one fixture of ONE body

Scenes without a `tol` of their own (DERIVED_SCENES) get one from the mini-solver alone: the largest position gap between a
float32 and a float64 run is its own rounding sensitivity there (`f32_f64_gap`); `tol` is the smallest of the classes 2e-5, 5e-5,
2e-4, 2e-3 that is at least 4 x that gap (x 2: the oracle rounds in another operation order; x 2 slack), 2e-3 at least where
several contacts are swept (creation order against canonical order).  A gap beyond 2e-3 / 4 is chaos: the scene is refused.
`measured` is the oracle's deviation [position, angle, velocity]: information, never an input to `tol`.
"""
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import box2d_mini as B  # noqa: E402

W, H = 2.0 * 25.0, 1.5 * 25.0
R_BOT = 0.0165 * 25.0

SCENES = {
    # single contacts: the order of the Gauss-Seidel sweep cannot matter -> tight tolerance
    'head_on': dict(kilobots=[[-0.5, 0.0, 0.0, 0.01, 0.0], [0.5, 0.02, math.pi, 0.01, 0.0]], objects=[], steps=40, tol=2e-5),
    'glancing': dict(kilobots=[[-0.45, -0.3, 0.6, 0.01, 0.2], [0.3, 0.25, -2.4, 0.008, -0.3]], objects=[], steps=40, tol=2e-5),
    'wall_left': dict(kilobots=[[-25.0 + 0.6, 3.0, math.pi - 0.5, 0.01, 0.1]], objects=[], steps=40, tol=2e-5),
    'wall_top': dict(kilobots=[[4.0, 18.75 - 0.55, 1.2, 0.01, -0.2]], objects=[], steps=40, tol=2e-5),
    'bot_pushes_box': dict(kilobots=[[-2.9, 0.7, 0.0, 0.01, 0.0]], objects=[dict(shape='box', hx=1.875, hy=1.875, x=0.0, y=0.0, theta=0.3, vx=0, vy=0, w=0)],
                           steps=60, tol=5e-5),
    'bot_pushes_disc': dict(kilobots=[[-2.6, 0.4, 0.0, 0.01, 0.0]], objects=[dict(shape='circle', r=1.875, x=0.0, y=0.0, theta=0.0, vx=0, vy=0, w=0)],
                            steps=60, tol=5e-5),
    'box_hits_wall': dict(kilobots=[[20.0, 15.0, 0.0, 0.0, 0.0]], objects=[dict(shape='box', hx=1.875, hy=1.25, x=3.0, y=-18.75 + 1.6, theta=0.25, vx=1.5, vy=-3.0, w=0.4)],
                          steps=40, tol=2e-4),
    'box_slides_on_wall': dict(kilobots=[[20.0, 15.0, 0.0, 0.0, 0.0]], objects=[dict(shape='box', hx=1.875, hy=1.25, x=-5.0, y=-18.75 + 1.25 + 0.015, theta=0.0, vx=4.0, vy=-0.5, w=0.0)],
                               steps=40, tol=2e-4),
    'box_slams_flat': dict(kilobots=[[20.0, 15.0, 0.0, 0.0, 0.0]], objects=[dict(shape='box', hx=1.875, hy=1.25, x=3.0, y=-18.75 + 1.25 + 0.25, theta=0.02, vx=2.5, vy=-8.0, w=1.2)],
                           steps=20, tol=2e-4),
    'disc_hits_wall': dict(kilobots=[[20.0, 15.0, 0.0, 0.0, 0.0]], objects=[dict(shape='circle', r=1.5, x=25.0 - 1.9, y=2.0, theta=0.0, vx=4.0, vy=2.0, w=0.0)],
                           steps=40, tol=5e-5),
    'disc_disc': dict(kilobots=[[20.0, 15.0, 0.0, 0.0, 0.0]], objects=[dict(shape='circle', r=1.5, x=-1.6, y=0.3, theta=0.0, vx=3.0, vy=0.0, w=0.0),
                                                                       dict(shape='circle', r=1.25, x=1.4, y=-0.5, theta=0.0, vx=-2.0, vy=0.5, w=1.0)], steps=40, tol=5e-5),
    'box_box': dict(kilobots=[[20.0, 15.0, 0.0, 0.0, 0.0]], objects=[dict(shape='box', hx=1.875, hy=1.875, x=-2.2, y=0.0, theta=0.0, vx=3.0, vy=0.0, w=0.0),
                                                                     dict(shape='box', hx=1.25, hy=1.25, x=1.3, y=0.6, theta=0.5, vx=-2.0, vy=0.0, w=0.0)], steps=40, tol=2e-4),
    # the continuous step (b2World::SolveTOI) against the walls: the same wall scenes with continuousPhysics on, a fast disc,
    # a kilobot that starts a hair outside the contact radius, a corner
    'wall_left__toi': dict(kilobots=[[-25.0 + 0.6, 3.0, math.pi - 0.5, 0.01, 0.1]], objects=[], steps=40, tol=2e-5, toi=True),
    'wall_top__toi': dict(kilobots=[[4.0, 18.75 - 0.55, 1.2, 0.01, -0.2]], objects=[], steps=40, tol=2e-5, toi=True),
    'wall_graze__toi': dict(kilobots=[[-25.0 + 0.4335, -2.0, math.pi / 2 + 0.05, 0.01, 0.0]], objects=[], steps=40, tol=2e-5, toi=True),
    'corner__toi': dict(kilobots=[[25.0 - 0.62, -18.75 + 0.6, -0.7, 0.01, 0.0]], objects=[], steps=60, tol=5e-5, toi=True),
    'disc_hits_wall__toi': dict(kilobots=[[20.0, 15.0, 0.0, 0.0, 0.0]], objects=[dict(shape='circle', r=1.5, x=25.0 - 1.9, y=2.0, theta=0.0, vx=4.0, vy=2.0, w=0.0)],
                                steps=40, tol=5e-5, toi=True),
    'fast_disc__toi': dict(kilobots=[[20.0, 15.0, 0.0, 0.0, 0.0]], objects=[dict(shape='circle', r=1.25, x=-25.0 + 3.2, y=-4.0, theta=0.0, vx=-16.0, vy=3.0, w=2.0)],
                           steps=30, tol=5e-5, toi=True),
    # several contacts: Box2D sweeps in contact-creation order, the oracle in its canonical key order -> looser tolerance
    'chain_of_three': dict(kilobots=[[-0.9, 0.0, 0.0, 0.01, 0.0], [-0.05, 0.03, 0.0, 0.0, 0.0], [0.8, -0.02, 0.0, 0.0, 0.0]], objects=[], steps=60, tol=2e-3),
    # sleeping (b2World doSleep = True, kilobots_env.py:45): `commands` = [[first step, [[v_cmd, omega_cmd] per kilobot]], ...]
    # replaces the per-kilobot commands from that step on.  Single contacts / no contacts: tight tolerance.
    'sleep_overlap_at_rest': dict(kilobots=[[0.0, 0.0, 0.0, 0.0, 0.0], [0.5, 0.0, 0.0, 0.0, 0.0], [12.5, 12.5, 0.0, 0.0, 0.0]], objects=[],
                                  steps=14, tol=2e-5, sleep=True),
    'sleep_and_wake_by_command': dict(kilobots=[[0.0, 0.0, 0.3, 0.01, 0.2], [6.0, 3.0, 0.0, 0.0, 0.0]], objects=[], steps=30, tol=2e-5, sleep=True, contact_free=True,
                                      commands=[[6, [[0.0, 0.0], [0.0, 0.0]]], [16, [[0.0003, 0.0], [0.0, 0.0]]], [24, [[0.008, -0.3], [0.0, 0.0]]]]),
    'sleeping_bot_woken_by_a_pusher': dict(kilobots=[[0.0, 0.0, 0.0, 0.0, 0.0], [1.5, 0.05, math.pi, 0.0, 0.0]], objects=[], steps=60, tol=5e-5, sleep=True,
                                           commands=[[8, [[0.0, 0.0], [0.01, 0.0]]]]),
    # b2Contact::Update: a contact that stops touching wakes both bodies -- kilobot 2 rests against kilobots 0 and 1, all three fall
    # asleep, then it is commanded away: its departure (the contacts end) wakes the two it leaves behind, whose sleep times restart
    'mover_leaves_a_sleeping_pair': dict(kilobots=[[0.0, 0.0, 0.0, 0.0, 0.0], [0.0, 0.82, 0.0, 0.0, 0.0], [0.71, 0.41, 0.0, 0.0, 0.0]], objects=[],
                                         steps=40, tol=5e-5, sleep=True, commands=[[14, [[0.0, 0.0], [0.0, 0.0], [0.01, 0.0]]]]),
    # ... and the case in which ONLY that rule wakes the sleeper: kilobot 0 creeps away from kilobot 1 below the sleep tolerance (its
    # tiny command re-wakes it every step, b2Body::SetLinearVelocity); both rest, fall asleep together at the end of step 10 -- the
    # step in which they stop touching -- and in step 11 the creeper's wake-up finds the contact gone: kilobot 1 is woken although no
    # island reaches it any more, and sleeps again five steps later
    'creeper_leaves_a_sleeper': dict(kilobots=[[0.0, 0.0, math.pi, 0.0002, 0.0], [0.8206, 0.0, 0.0, 0.0, 0.0]], objects=[], steps=20, tol=2e-5, sleep=True),
    'disc_coasts_to_sleep': dict(kilobots=[[20.0, 15.0, 0.0, 0.0, 0.0]], objects=[dict(shape='circle', r=1.5, x=0.0, y=0.0, theta=0.0, vx=0.6, vy=0.2, w=0.3)],
                                 steps=70, tol=5e-5, sleep=True, contact_free=True),
    # kilobots of different classes: fixture density 2 (SimpleVelocityControlKilobot, kilobot.py:214) against density 1 (Kilobot,
    # :25): a sixth column gives the density; the light one is commanded (0, 0) like a kilobot with both motors off
    'heavy_pushes_light': dict(kilobots=[[-0.6, 0.0, 0.0, 0.01, 0.0, 2.0], [0.45, 0.03, 0.0, 0.0, 0.0, 1.0]], objects=[], steps=50, tol=2e-5),
    'heavy_light_heavy_chain': dict(kilobots=[[-0.9, 0.0, 0.0, 0.01, 0.0, 2.0], [-0.05, 0.03, 0.0, 0.0, 0.0, 1.0], [0.8, -0.02, 0.0, 0.0, 0.0, 2.0]],
                                    objects=[], steps=60, tol=2e-3),
    'two_bots_push_box': dict(kilobots=[[-2.9, 0.9, 0.0, 0.01, 0.0], [-2.9, -0.8, 0.0, 0.01, 0.0]],
                              objects=[dict(shape='box', hx=1.875, hy=1.875, x=0.0, y=0.0, theta=0.0, vx=0, vy=0, w=0)], steps=60, tol=2e-3),
}


PARKED = [[20.0, 15.0, 0.0, 0.0, 0.0]]          # a kilobot out of the way (a scene needs one)


def _obj(shape, x, y, theta=0.0, vx=0.0, vy=0.0, w=0.0, **kw):
    if shape not in ('circle', 'box'):
        kw.setdefault('width', 0.15)
        kw.setdefault('height', 0.15)
    return dict(shape=shape, x=x, y=y, theta=theta, vx=vx, vy=vy, w=w, **kw)


# The 0.15 m Triangle in world units, in the order of b2PolygonShape::Set: (1.25, -1.25), (1.25, 2.5), (-2.5, -1.25).
# The 0.15 m LForm: an upright bar x -0.47 .. 1.41, y -0.31 .. 2.19 on a lying bar x -2.34 .. 1.41, y -1.56 .. -0.31; the
# inner corner is at (-0.47, -0.31), and both bars end at x = 1.41.  TForm: a bar 1.875 x 3.75 on the right, a stem 1.875 x 1.25
# to the left.  CForm: a spine on the right and two arms whose mouth opens to the left, 2 units wide at the tips, 1.25 inside.
DERIVED_SCENES = {
    # ---- discrete step (continuousPhysics off): polygons made by b2PolygonShape::Set
    'triangle_face_push': dict(kilobots=[[1.78, 1.5, math.pi, 0.01, 0.0]], objects=[_obj('Triangle', 0.0, 0.0)], steps=60),
    'triangle_vertex_push': dict(kilobots=[[1.7, 2.75, math.pi, 0.01, 0.0]], objects=[_obj('Triangle', 0.0, 0.0)], steps=60),
    'triangle_hits_wall': dict(kilobots=PARKED, objects=[_obj('Triangle', 3.0, -18.75 + 1.7218 + 0.3, 0.2, 0.8, -1.5, 0.3)], steps=40),
    # an irregular convex quad, outline given CLOCKWISE and starting at its TOP-LEFT vertex
    'quad_set_order_hits_box': dict(kilobots=PARKED, objects=[
        _obj('polygon', -2.3, 0.2, 0.2, 3.0, 0.0, 0.0, verts=[[-0.5, 0.4], [0.3, 0.5], [0.5, -0.3], [-0.4, -0.5]]),
        _obj('box', 1.4, 0.0, 0.45, -1.0, 0.0, 0.0, hx=1.25, hy=1.25)], steps=40),
    # ---- compound bodies
    'lform_free_flight': dict(kilobots=PARKED, objects=[_obj('LForm', 0.0, 0.0, 0.4, 2.0, 1.0, 1.5)], steps=40, contact_free=True),
    # (the parts of an L or a T are rectangles, so the reference's recentring puts the origin ON the centre of mass; the arms of
    # the C are trapezoids, its local centre is not zero, and the origin circles the centre of mass while the body spins)
    'cform_free_flight': dict(kilobots=PARKED, objects=[_obj('CForm', 0.0, 0.0, -0.7, -1.5, 2.0, -2.5)], steps=40, contact_free=True),
    'lform_inner_corner': dict(kilobots=[[-1.04, 0.26, -math.pi / 4, 0.01, 0.0]], objects=[_obj('LForm', 0.0, 0.0)], steps=60,
                               several_contacts=True),
    'tform_hits_wall': dict(kilobots=PARKED, objects=[_obj('TForm', 2.0, -18.75 + 2.6, 0.5, 0.5, -2.0, 0.2)], steps=60,
                            several_contacts=True),
    'cform_hits_box': dict(kilobots=PARKED, objects=[_obj('CForm', 1.0, 0.0), _obj('box', -2.6, 0.1, 0.0, 2.0, 0.0, 0.0, hx=0.7, hy=0.7)],
                           steps=60, several_contacts=True),
    # ---- continuous step of polygons against the walls (b2TimeOfImpact on b2Distance / b2SeparationFunction)
    'box_thrown__toi_a': dict(kilobots=PARKED, objects=[_obj('box', 20.0, 2.5, 0.3, 12.0, 1.0, 3.0, hx=1.875, hy=1.875)], steps=20, toi=True),
    'box_thrown__toi_b': dict(kilobots=PARKED, objects=[_obj('box', 20.0, 2.5, 0.0, 12.0, 1.0, 0.0, hx=1.875, hy=1.875)], steps=20, toi=True),
    'box_thrown__toi_c': dict(kilobots=PARKED, objects=[_obj('box', 20.0, 2.5, math.pi / 4, 12.0, 1.0, -5.0, hx=1.875, hy=1.875)], steps=20, toi=True),
    'triangle_thrown__toi': dict(kilobots=PARKED, objects=[_obj('Triangle', 0.0, 18.75 - 4.5, 0.3, 1.0, 12.0, 4.0)], steps=20, toi=True),
    # a trapezoid: its centre of mass lies 0.42 units from the body origin (the vertex mean), so the swept transform
    # p = c - R localCenter of b2Sweep::GetTransform matters as soon as it spins
    'trapezoid_thrown__toi': dict(kilobots=PARKED, objects=[_obj('polygon', 20.0, -3.0, 0.4, 12.0, -1.0, 4.0,
                                                                 verts=[[-0.5, -0.5], [0.5, -0.1], [0.5, 0.1], [-0.5, 0.5]])], steps=20, toi=True),
    'lform_thrown__toi': dict(kilobots=PARKED, objects=[_obj('LForm', 20.0, 0.0, 0.02, 12.0, 0.5, 0.3)], steps=20, toi=True,
                              several_contacts=True),
    'cform_thrown__toi': dict(kilobots=PARKED, objects=[_obj('CForm', -20.0, 1.0, 0.02, -12.0, 0.5, 0.3)], steps=20, toi=True,
                              several_contacts=True),
    'box_rests_on_wall__toi': dict(kilobots=PARKED, objects=[_obj('box', 0.0, -18.75 + 1.875 + 0.015, 0.0, hx=1.875, hy=1.875)], steps=30, toi=True),
    'box_into_corner__toi': dict(kilobots=[[0.0, 0.0, 0.0, 0.0, 0.0]], objects=[_obj('box', 25.0 - 5.0, 18.75 - 5.0, 0.2, 9.0, 9.0, 4.0, hx=1.875, hy=1.875)],
                                 steps=20, toi=True),
}


def sub_polygons(o):
    """The convex parts of an object given by class, in world units relative to the body origin: the unit outline is scaled
    so that its bounding box becomes width x height, and the origin is put on the area-weighted mean of the parts' vertex
    means (the reference's Polygon.__init__, in double); x 25 in double, rounded to float32 only by b2PolygonShape::Set."""
    if o['shape'] == 'polygon':
        unit = [o['verts']]
    else:
        sys.path.insert(0, ROOT)
        from gym_kilobots_amd.lib import body as lib_body
        unit = getattr(lib_body, o['shape'])._shape_vertices()
    parts = [[(float(x), float(y)) for x, y in part] for part in unit]
    xs = [x for part in parts for x, _ in part]
    ys = [y for part in parts for _, y in part]
    sx, sy = o['width'] / (max(xs) - min(xs)), o['height'] / (max(ys) - min(ys))
    parts = [[(x * sx, y * sy) for x, y in part] for part in parts]
    cx = cy = total = 0.0
    for part in parts:
        n = len(part)
        area = 0.5 * abs(sum(part[i][0] * part[i - 1][1] - part[i][1] * part[i - 1][0] for i in range(n)))
        cx += area * sum(x for x, _ in part) / n
        cy += area * sum(y for _, y in part) / n
        total += area
    cx, cy = cx / total, cy / total
    return [[((x - cx) * 25.0, (y - cy) * 25.0) for x, y in part] for part in parts]


def shapes_of(o):
    if o['shape'] == 'circle':
        return [B.Circle(o['r'])]
    if o['shape'] == 'box':
        return [B.Polygon.box(o['hx'], o['hy'])]
    return [B.Polygon.set(part) for part in sub_polygons(o)]


def run(scene, damping='pade', dt=0.1, vel_iters=10, pos_iters=10, observe=None):
    """One scene through the mini-solver in its current precision: (trajectory, touched).  `observe(k, world)` is called
    after every step."""
    f = B.f32
    w = B.World(damping=damping, continuous=bool(scene.get('toi')), allow_sleep=bool(scene.get('sleep')))
    table = w.create_body(dynamic=False)
    x0, x1, y0, y1 = -W / 2, W / 2, -H / 2, H / 2
    for a, b in (((x0, y1), (x0, y0)), ((x0, y0), (x1, y0)), ((x1, y0), (x1, y1)), ((x1, y1), (x0, y1))):   # kilobots_env.py:48-51
        table.create_fixture(B.Edge(a, b), density=0.0, friction=0.2)
    bots, objs = [], []
    for kb in scene['kilobots']:
        x, y, th, v, om = kb[:5]
        b = w.create_body(position=(x, y), angle=th, linear_damping=0.8, angular_damping=0.8)
        b.create_fixture(B.Circle(R_BOT), density=kb[5] if len(kb) > 5 else 2.0, friction=0.0, restitution=0.0)
        bots.append([b, f(v), f(om)])
    for o in scene['objects']:
        b = w.create_body(position=(o['x'], o['y']), angle=o['theta'], linear_damping=0.8, angular_damping=0.8)
        for shape in shapes_of(o):
            b.create_fixture(shape, density=2.0, friction=0.01, restitution=0.0)
        b.v, b.w = B.V(o['vx'], o['vy']), f(o['w'])
        objs.append(b)
    traj = []
    for k in range(scene['steps']):
        for first, cmds in scene.get('commands', []):
            if first == k:
                for bot, (v, om) in zip(bots, cmds):
                    bot[1], bot[2] = f(v), f(om)
        for b, v, om in bots:                 # SimpleVelocityControlKilobot.step, kilobot.py:253-258 (assignments through the
            sp = v * f(25.0)                  # b2Body setters, which wake a sleeping body iff the value is non-zero)
            b.set_angular_velocity(om)
            b.set_linear_velocity(B.V(f(math.cos(float(b.a))) * sp, f(math.sin(float(b.a))) * sp))
        w.step(dt, vel_iters, pos_iters)
        rec = {'kilobots': [[float(b.position.x), float(b.position.y), float(b.angle)] for b, _, _ in bots],
               'objects': [[float(b.position.x), float(b.position.y), float(b.angle), float(b.v.x), float(b.v.y), float(b.w)] for b in objs]}
        if scene.get('sleep'):                # m_sleepTime, -1 = asleep (the encoding of kb_buffers.sleep_time)
            rec['sleep'] = [float(b.sleep_time) if b.awake else -1.0 for b, _, _ in bots]
            rec['osleep'] = [float(b.sleep_time) if b.awake else -1.0 for b in objs]
        traj.append(rec)
        if observe is not None:
            observe(k, w)
    touched = any(c.touching for c in w.contacts)
    return traj, touched


TOL_CLASSES = (2e-5, 5e-5, 2e-4, 2e-3)
SEVERAL_CONTACTS_TOL = 2e-3


def position_gap(ta, tb):
    """largest difference of any kilobot or object position between two trajectories"""
    gap = 0.0
    for ra, rb in zip(ta, tb):
        for key in ('kilobots', 'objects'):
            for pa, pb in zip(ra[key], rb[key]):
                gap = max(gap, abs(pa[0] - pb[0]), abs(pa[1] - pb[1]))
    return gap


def derive_tol(name, scene):
    """(trajectory, f32_f64_gap, tol) of a scene without a tolerance of its own; raises if the scene is chaotic."""
    assert B.precision() == 32
    traj, _ = run(scene)
    B.set_precision(64)
    try:
        traj64, _ = run(scene)
    finally:
        B.set_precision(32)
    gap = position_gap(traj, traj64)
    if 4.0 * gap > TOL_CLASSES[-1]:
        raise SystemExit('%s: the float32 and float64 runs of the mini-solver are %.3e apart, more than 2e-3 / 4: the scene is '
                         'chaotic; make it shorter or slower' % (name, gap))
    tol = min(t for t in TOL_CLASSES if t >= 4.0 * gap)
    if scene.get('several_contacts'):
        tol = max(tol, SEVERAL_CONTACTS_TOL)
    return traj, gap, tol


def measure(entry):
    """The oracle's largest deviation from the trajectory of a finished fixture entry: [position, angle, velocity]."""
    sys.path.insert(0, ROOT)
    from tests import mini_scenes as MS
    o = MS.oracle_for(entry)
    worst = [0.0, 0.0, 0.0]
    for ref in entry['trajectory']:
        o.step(1)
        worst = [max(a, b) for a, b in zip(worst, MS.deviation(o, ref, len(entry['objects'])))]
    return worst


def generate(verbose=True):
    out = {'_about': 'trajectories of tools/box2d_mini.py (independent restatement of Box2D 2.3.1 b2World::Step, continuousPhysics off); '
                     'made by tools/gen_mini_solver_golden.py; world units (metres x 25)', 'scenes': {}}
    for name, sc in SCENES.items():
        for damping in ('pade', 'linear'):
            if damping == 'linear' and name not in ('head_on', 'box_hits_wall'):
                continue
            traj, _ = run(sc, damping)
            key = name if damping == 'pade' else name + '__linear_damping'
            out['scenes'][key] = dict(sc, damping=damping, trajectory=traj)
            if verbose:
                print(key, 'final', traj[-1]['kilobots'][0], traj[-1]['objects'][:1])
    derived = {}
    for name, sc in DERIVED_SCENES.items():
        assert sc['steps'] <= 80 and 'tol' not in sc and name not in out['scenes']
        traj, gap, tol = derive_tol(name, sc)
        entry = dict(sc, damping='pade', f32_f64_gap=gap, tol=tol, trajectory=traj)
        entry['measured'] = measure(entry)
        derived[name] = entry
        if verbose:
            print('%-28s gap %.2e  tol %.0e  measured pos %.2e ang %.2e vel %.2e' % ((name, gap, tol) + tuple(entry['measured'])))
    return out, derived


def _without_measured(entry):
    return json.dumps({k: v for k, v in entry.items() if k != 'measured'})


def main(argv):
    """The first generation goes to mini_solver.json as ever; the derived scenes go to mini_solver_polygons.json (everything
    but the trajectories, readable) and mini_solver_polygons.npz (the trajectories as float32 arrays, which is what they are)."""
    sys.path.insert(0, ROOT)
    from tests import mini_scenes as MS
    p = os.path.join(MS.GOLDEN, 'mini_solver.json')
    out, derived = generate(verbose='--check' not in argv)
    if '--check' in argv:
        # everything the mini-solver determines is compared byte for byte (`measured` comes from the oracle: information)
        have = MS.load_fixture()
        bad = [] if json.dumps(out) == open(p).read() else ['mini_solver.json']
        bad += [k for k in sorted(set(have) - set(out['scenes']) | set(derived))
                if k not in have or k not in derived or _without_measured(have[k]) != _without_measured(derived[k])]
        if bad:
            raise SystemExit('the committed fixture differs from a fresh run in: %s' % ', '.join(bad))
        print('ok: mini_solver.json reproduces byte for byte, the %d derived scenes value for value; their tolerances obey the '
              '4 x gap rule' % len(derived))
        return
    json.dump(out, open(p, 'w'))
    meta = {'_about': 'the polygon / compound / polygon-TOI scenes of tools/gen_mini_solver_golden.py: description, derived tolerance, '
                      'float32 / float64 gap of the mini-solver, measured deviation of the oracle [position, angle, velocity]; '
                      'trajectories in mini_solver_polygons.npz', 'scenes': {k: {a: b for a, b in v.items() if a != 'trajectory'} for k, v in derived.items()}}
    with open(os.path.join(MS.GOLDEN, 'mini_solver_polygons.json'), 'w') as f:        # one scene per line
        f.write('{"_about": %s, "scenes": {\n%s\n}}\n' % (json.dumps(meta['_about']), ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(v)) for k, v in meta['scenes'].items())))
    arrays = {}
    for k, v in derived.items():
        for part in ('kilobots', 'objects'):
            arrays[k + '.' + part] = np.array([rec[part] for rec in v['trajectory']], np.float64).astype(np.float32)
            assert np.array_equal(arrays[k + '.' + part].astype(np.float64), np.array([rec[part] for rec in v['trajectory']]))
    np.savez_compressed(os.path.join(MS.GOLDEN, 'mini_solver_polygons.npz'), **arrays)
    for f in ('mini_solver.json', 'mini_solver_polygons.json', 'mini_solver_polygons.npz'):
        print('wrote', f, os.path.getsize(os.path.join(MS.GOLDEN, f)), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1:])
