"""Row a10 / f1 (the Box2D solver): the oracle against an INDEPENDENT second derivation of Box2D's discrete step.

oracle/kb_oracle.c and the HIP kernel are twins of one restatement, so their bit-exact agreement cannot reveal a shared
transcription error of Box2D.  tools/box2d_mini.py is a separate float32 restatement written in Box2D's own structure
(bodies, fixtures, persistent contacts in creation order, b2ContactSolver per contact); tests/golden/mini_solver.json holds
its trajectories for small scenes (circle-circle, circle-wall, polygon-circle with lever arm, box-wall with the two-point
block solver and friction, disc-disc with friction, box-box, and -- scenes `*__toi` -- the continuous step of kilobots and
discs against the walls: b2TimeOfImpact, Advance, the TOI sub-solve; without it the oracle is 150 .. 18 000 tolerances away).  The oracle must follow them within a float32 tolerance
(stated per scene in the fixture: 2e-5 .. 2e-4 world units = 1 .. 8 micrometres for single-contact scenes, where the
sweep order cannot matter; 2e-3 for scenes with several contacts, where Box2D's creation order and the oracle's canonical
order legitimately differ).  box2d-py itself cannot be installed here: row a10 stays "parity unpinned" (DESIGN.md).

The second generation of scenes (those with `f32_f64_gap` in the fixture) covers what the first left to known-answer and
qualitative checks: polygons made by b2PolygonShape::Set (Triangle, an irregular quad given clockwise from its top-left
vertex), compound bodies (LForm, TForm, CForm: mass data over several fixtures, a centre of mass off the body origin, no
contacts inside a body, warm starting per fixture) and the continuous step of polygons against the walls, where the
mini-solver runs Box2D's general b2TimeOfImpact on b2Distance and the oracle its closed-form support-vertex distance.  Those
scenes are described by object class and reach the oracle through the project's own translation (tests/mini_scenes.py), which
a test compares vertex for vertex with the mini-solver's own Set.  Their tolerance is derived by the generator from the
mini-solver alone (4 x its float32 / float64 gap, rounded up to a class; tools/gen_mini_solver_golden.py); the oracle's measured
deviation stands next to it as information.  Vacuity guards: a `__toi` polygon scene must leave its trajectory by more than
its tolerance when the continuous step is off, a compound scene must touch with two fixtures of one body at some step, the
quad must get a two-point manifold."""
import os
import sys

import numpy as np
import pytest

from tests import mini_scenes as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = MS.FIX
_oracle_for = MS.oracle_for
TOL_CLASSES = (2e-5, 5e-5, 2e-4, 2e-3)
COMPOUND = ('LForm', 'TForm', 'CForm')


def _tools():
    if os.path.join(ROOT, 'tools') not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import box2d_mini
    import gen_mini_solver_golden
    return gen_mini_solver_golden, box2d_mini


@pytest.mark.parametrize('name', sorted(FIX))
def test_oracle_follows_the_independent_solver(name):
    sc = FIX[name]
    o = _oracle_for(sc)
    tol = sc['tol']
    touched = two_fixtures = two_points = False
    slept = woke = False
    guard_fixtures = 'f32_f64_gap' in sc
    fixture_body = MS.fixtures_of(sc['objects'])[1]
    for k, ref in enumerate(sc['trajectory']):
        for first, cmds in sc.get('commands', []):            # the scene's commands change at these steps
            if first == k:
                o.set_actions(np.array(cmds, np.float32)[None])
        o.step(1)
        if sc.get('sleep'):
            # b2Body::m_sleepTime of every body, -1 = asleep: the same substep falls asleep / wakes in both derivations
            for got_s, want_s in ((o.sleep_time[0], ref['sleep']), (o.osleep[0][:len(sc['objects'])], ref['osleep'])):
                want_s = np.array(want_s, np.float64)
                assert np.array_equal(np.asarray(got_s) < 0, want_s < 0), (name, k, 'asleep flags', got_s, want_s)
                assert np.abs(np.asarray(got_s, np.float64) - want_s).max(initial=0.0) <= 1e-6, (name, k, 'sleep time')
            now = np.array(ref['sleep'] + ref['osleep']) < 0
            slept |= bool(now.any())
            woke |= slept and not now.all() and k > 0 and bool((np.array(sc['trajectory'][k - 1]['sleep'] + sc['trajectory'][k - 1]['osleep']) < 0)[~now].any())
        got = np.stack([o.x[0], o.y[0], o.theta[0]], -1).astype(np.float64)
        want = np.array(ref['kilobots'])
        assert np.abs(got[:, :2] - want[:, :2]).max() <= tol, (name, k, 'kilobot position', got, want)
        assert np.abs(got[:, 2] - want[:, 2]).max() <= 10 * tol, (name, k, 'kilobot angle')
        if sc['objects']:
            g = np.stack([o.ox[0], o.oy[0], o.otheta[0], o.ovx[0], o.ovy[0], o.ow[0]], -1).astype(np.float64)
            w = np.array(ref['objects'])
            assert np.abs(g[:, :2] - w[:, :2]).max() <= tol, (name, k, 'object position', g, w)
            assert np.abs(g[:, 2] - w[:, 2]).max() <= 10 * tol, (name, k, 'object angle', g, w)
            assert np.abs(g[:, 3:] - w[:, 3:]).max() <= 200 * tol, (name, k, 'object velocity', g, w)
        nb, nw, no = o.count_contacts(0, True)
        touched |= (nb + nw + no) > 0
        if guard_fixtures:
            hit = MS.touched_fixtures(o)
            two_fixtures |= any(len({f for f in hit if f < len(fixture_body) and fixture_body[f] == b}) >= 2 for b in set(fixture_body))
            two_points |= MS.two_point_manifold(o)
    assert touched or sc.get('contact_free'), 'the scene never made a contact'
    # vacuity guards: a compound body met something with two of its fixtures at once; the quad got a two-point manifold
    if guard_fixtures and any(ob['shape'] in COMPOUND for ob in sc['objects']) and not sc.get('contact_free'):
        assert two_fixtures, 'no step had contacts on two fixtures of one body'
    if name == 'quad_set_order_hits_box':
        assert two_points, 'no two-point manifold'
    if sc.get('sleep'):
        assert slept, 'nothing fell asleep'
        if 'wake' in name or 'woken' in name:
            assert woke, 'nothing woke up'
    assert int(o.status.max()) == 0


def test_fixture_is_what_the_mini_solver_produces():
    """The committed fixture equals a fresh run of tools/box2d_mini.py (four scenes, bit for bit through JSON): a discrete and
    a wall scene of the first generation, one polygon-TOI scene and one compound scene."""
    G, _ = _tools()
    for name in ('head_on', 'box_hits_wall'):
        traj, touched = G.run(G.SCENES[name])
        assert touched
        assert traj == FIX[name]['trajectory']
    for name in ('triangle_thrown__toi', 'lform_inner_corner'):
        traj, gap, tol = G.derive_tol(name, G.DERIVED_SCENES[name])
        assert traj == FIX[name]['trajectory']
        assert gap == FIX[name]['f32_f64_gap'] and tol == FIX[name]['tol']


@pytest.mark.parametrize('name', sorted(n for n in FIX if any(o['shape'] not in ('circle', 'box') for o in FIX[n]['objects'])))
def test_scene_shapes_reach_the_oracle_in_the_order_of_set(name):
    """The configuration the oracle and the device get for a scene (lib.body: scaling, centring, x 25 in double, hull order)
    holds, fixture for fixture and vertex for vertex as float32, what the mini-solver's own b2PolygonShape::Set makes of the
    generator's restatement of the outline: same start vertex (right-most, lowest on a tie), same direction, same numbers.
    The physics cannot tell a rotated vertex list from the right one (only feature ids and tie-breaks move), this can."""
    G, _ = _tools()
    sc = FIX[name]
    specs, fixture_body = MS.fixtures_of(sc['objects'])
    k = 0
    for i, ob in enumerate(sc['objects']):
        shapes = G.shapes_of(ob)
        assert fixture_body[k:k + len(shapes)] == [i] * len(shapes)
        for shape in shapes:
            if ob['shape'] not in ('circle', 'box'):
                got = np.array(specs[k][2], np.float64).astype(np.float32)
                want = np.array([v.tup() for v in shape.vertices], np.float32)
                assert specs[k][0] == 2 and got.shape == want.shape and np.array_equal(got, want), (name, i, got, want)
            k += 1
    assert k == len(specs)


def test_derived_tolerances_obey_the_gap_rule():
    """Every scene with a derived tolerance carries the mini-solver's float32 / float64 gap and the oracle's measured deviation;
    its tolerance is the smallest class that is at least 4 x the gap (2e-3 at least where several contacts are swept).  No scene
    needs the documented-deviation class of one linear slop, the arena-corner scene included."""
    derived = [n for n in FIX if 'f32_f64_gap' in FIX[n]]
    assert len(derived) >= 15
    for name in derived:
        sc = FIX[name]
        assert len(sc['trajectory']) <= 80 and len(sc['measured']) == 3
        assert 4.0 * sc['f32_f64_gap'] <= TOL_CLASSES[-1], name
        want = min(t for t in TOL_CLASSES if t >= 4.0 * sc['f32_f64_gap'])
        if sc.get('several_contacts'):
            want = max(want, 2e-3)
        assert sc['tol'] == want, name


@pytest.mark.parametrize('name', sorted(n for n in FIX if '__toi' in n and 'f32_f64_gap' in FIX[n]))
def test_toi_scenes_have_a_continuous_step_event(name):
    """A `__toi` scene that never triggers a TOI event would pass with the continuous step broken: the oracle run with
    toi_walls = 0 must leave the trajectory by more than the scene's tolerance (position).  The box at rest on a wall is the
    opposite case: the continuous step must not move it, bit for bit.  (The guard covers the polygon scenes, whose tolerance
    is derived; of the six older kilobot / disc scenes two are no-event scenes on purpose -- `wall_graze__toi` holds the exact
    no-event test -- and stay pinned by their trajectories.)"""
    sc = FIX[name]
    on, off = MS.oracle_for(sc), MS.oracle_for(dict(sc, toi=False))
    worst, same = 0.0, True
    for ref in sc['trajectory']:
        on.step(1)
        off.step(1)
        worst = max(worst, MS.deviation(off, ref, len(sc['objects']))[0])
        same &= all(np.array_equal(getattr(on, f), getattr(off, f)) for f in ('x', 'y', 'theta', 'ox', 'oy', 'otheta', 'ovx', 'ovy', 'ow'))
    if name == 'box_rests_on_wall__toi':
        assert same
        first, last = sc['trajectory'][0]['objects'][0], sc['trajectory'][-1]['objects'][0]
        assert first == last and first[3:] == [0.0, 0.0, 0.0], 'the resting box moved'
    else:
        assert worst > sc['tol'], (name, worst)
