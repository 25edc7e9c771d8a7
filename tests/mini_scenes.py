"""From a scene of tests/golden/mini_solver.json to the configuration and the initial state of a simulator: shared by the
CPU test (oracle), the GPU test (HIP path) and tools/gen_mini_solver_golden.py (which measures the oracle's deviation).

Circles and boxes are described by their size in world units.  Every other object is described by its CLASS
(`Triangle`, `LForm`, `TForm`, `CForm`, or `polygon` with an explicit unit outline `verts`) and a width and height in metres,
and goes through the project's own translation of those classes: gym_kilobots_amd.lib.body scales and recentres the outline
and puts every convex part into the vertex order of b2PolygonShape::Set (`_shape_spec`), and the fixture list becomes
`obj_shape / obj_nverts / obj_verts / num_fixtures / obj_fixture_body` the way KilobotsEnv._upload_scene fills them.  The
mini-solver gets the same outlines through its own b2PolygonShape::Set, so a scene that holds also checks that translation."""
import json
import os

import numpy as np

from gym_kilobots_amd.lib import body as lib_body
from oracle import oracle as O

KEY_OBJ, KEY_EMPTY = 0x20000, 0xFFFFFFFF          # warm-start key of a kilobot-fixture contact: KEY_OBJ + fixture
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load_fixture():
    """All scenes by name.  mini_solver.json holds the first generation whole; the polygon scenes keep their description,
    tolerance, gap and measured deviation in mini_solver_polygons.json and their trajectories (float32, exact) as arrays
    `<scene>.kilobots` [steps, N, 3] and `<scene>.objects` [steps, M, 6] in mini_solver_polygons.npz."""
    scenes = json.load(open(os.path.join(GOLDEN, 'mini_solver.json')))['scenes']
    meta = json.load(open(os.path.join(GOLDEN, 'mini_solver_polygons.json')))['scenes']
    with np.load(os.path.join(GOLDEN, 'mini_solver_polygons.npz')) as z:
        for name, sc in meta.items():
            kb, ob = z[name + '.kilobots'].astype(np.float64), z[name + '.objects'].astype(np.float64)
            assert name not in scenes and len(kb) == len(ob) == sc['steps']
            scenes[name] = dict(sc, trajectory=[{'kilobots': kb[k].tolist(), 'objects': ob[k].tolist()} for k in range(len(kb))])
    return scenes


FIX = load_fixture()      # what the oracle test and the GPU test of the scenes parametrise over


def _body_of(o):
    """The lib.body object of a scene object described by class (None for the plain circle / box descriptions)."""
    if o['shape'] in ('circle', 'box'):
        return None
    world = lib_body.World()
    if o['shape'] == 'polygon':
        outline = np.array([o['verts']], dtype=np.float64)
        cls = type('ScenePolygon', (lib_body.Polygon,), {'_shape_vertices': staticmethod(lambda: outline.copy())})
    else:
        cls = getattr(lib_body, o['shape'])
    return cls(width=o['width'], height=o['height'], world=world)


def fixtures_of(objs):
    """[(kb_shape, radius [m], vertices [world units])] over all objects and the body index of every fixture."""
    specs, fixture_body = [], []
    for i, o in enumerate(objs):
        b = _body_of(o)
        if b is not None:
            fx = b._shape_spec()
        elif o['shape'] == 'circle':
            fx = [(O.SHAPE_CIRCLE, o['r'] / 25.0, [])]
        else:
            fx = [(O.SHAPE_BOX, 0.0, [[o['hx'], o['hy']]])]
        specs.extend(fx)
        fixture_body.extend([i] * len(fx))
    return specs, fixture_body


def config_kw(sc):
    """The kb_config overrides of a scene (the same for the oracle and the device)."""
    objs = sc['objects']
    kw = dict(toi_walls=1 if sc.get('toi') else 0, damping_model=1 if sc['damping'] == 'linear' else 0,
              allow_sleep=1 if sc.get('sleep') else 0)
    if objs:
        specs, fixture_body = fixtures_of(objs)
        pad = O.MAX_OBJECTS - len(specs)
        assert pad >= 0
        kw.update(num_objects=len(objs), num_fixtures=len(specs), obj_fixture_body=fixture_body + [0] * pad,
                  obj_shape=[sp[0] for sp in specs] + [0] * pad,
                  obj_nverts=[4 if sp[0] == O.SHAPE_BOX else len(sp[2]) for sp in specs] + [0] * pad,
                  obj_radius=[sp[1] for sp in specs] + [0.075] * pad,
                  obj_verts=[sp[2] if sp[2] else [[0.0, 0.0]] for sp in specs] + [[[0.0, 0.0]]] * pad)
    kb = np.array(sc['kilobots'], np.float64)
    mixed = kb.shape[1] > 5                      # a density column: kilobots of different classes (KB_DRIVE_MIXED)
    if mixed:
        kw.update(mode_density=[2.0, 2.0, 1.0, 1.0, 1.0])
    return kw, kb, mixed


def oracle_for(sc):
    kw, kb, mixed = config_kw(sc)
    objs = sc['objects']
    o = O.OracleSim(O.default_config(1, len(kb), O.DRIVE_MIXED if mixed else O.DRIVE_VELOCITY, **kw))
    if mixed:                                    # density 2: velocity control; density 1: the motor law with both motors off
        o.bot_mode[0] = np.where(kb[:, 5] == 2.0, O.DRIVE_VELOCITY, O.DRIVE_MOTORS)
        o.motor_l[...] = 0
        o.motor_r[...] = 0
    o.x[0], o.y[0], o.theta[0] = kb[:, 0].astype(np.float32), kb[:, 1].astype(np.float32), kb[:, 2].astype(np.float32)
    o.set_actions(kb[None, :, 3:5].astype(np.float32))
    for m, ob in enumerate(objs):
        o.ox[0, m], o.oy[0, m], o.otheta[0, m] = ob['x'], ob['y'], ob['theta']
        o.ovx[0, m], o.ovy[0, m], o.ow[0, m] = ob['vx'], ob['vy'], ob['w']
    return o


def sim_for(sc, **sim_kw):
    import torch
    from gym_kilobots_amd.sim import KilobotSim
    kw, kb, mixed = config_kw(sc)
    objs = sc['objects']
    g = KilobotSim(1, len(kb), O.DRIVE_MIXED if mixed else O.DRIVE_VELOCITY, **sim_kw, **kw)
    dev = g.x.device
    if mixed:
        g.bot_mode.copy_(torch.tensor(np.where(kb[None, :, 5] == 2.0, O.DRIVE_VELOCITY, O.DRIVE_MOTORS), dtype=torch.uint8, device=dev))
        g.motor_l.zero_()
        g.motor_r.zero_()
    g.x.copy_(torch.tensor(kb[None, :, 0], dtype=torch.float32, device=dev))
    g.y.copy_(torch.tensor(kb[None, :, 1], dtype=torch.float32, device=dev))
    g.theta.copy_(torch.tensor(kb[None, :, 2], dtype=torch.float32, device=dev))
    g.forget_contacts()
    g.set_actions(torch.tensor(kb[None, :, 3:5], dtype=torch.float32, device=dev).contiguous())
    for name, key in (('ox', 'x'), ('oy', 'y'), ('otheta', 'theta'), ('ovx', 'vx'), ('ovy', 'vy'), ('ow', 'w')):
        if objs:
            getattr(g, name).copy_(torch.tensor([[o[key] for o in objs]], dtype=torch.float32, device=dev))
    return g


def touched_fixtures(o):
    """The fixtures of env 0 of an OracleSim that hold an active manifold (with another fixture or a wall) or a kilobot
    contact after the last step, as a set of fixture indices."""
    hit = set()
    acc = o.ows_acc[0]                           # [fixture][partner fixture 0..7 | 8 + wall][id, n, t, id, n, t]
    for f in range(O.MAX_OBJECTS):
        for col in range(O.OWS_COLS):
            if acc[f, col, 0] >= 0 or acc[f, col, 3] >= 0:
                hit.add(f)
                if col < O.MAX_OBJECTS:
                    hit.add(col)
    used = o.ws_key[0][:int(o.ws_cnt[0].astype(np.int64).sum())]
    for key in used:
        if KEY_OBJ <= int(key) < KEY_EMPTY:
            hit.add(int(key) - KEY_OBJ)
    return hit


def two_point_manifold(o):
    """True if env 0 of an OracleSim holds a manifold with two points after the last step."""
    acc = o.ows_acc[0]
    return bool(((acc[:, :, 0] >= 0) & (acc[:, :, 3] >= 0)).any())


def deviation(o, ref, n_obj):
    """(position, angle, velocity) deviation of env 0 of a simulator's numpy state from one fixture record."""
    want = np.array(ref['kilobots'])
    got = np.stack([o.x[0], o.y[0], o.theta[0]], -1).astype(np.float64)
    pos, ang, vel = np.abs(got[:, :2] - want[:, :2]).max(), np.abs(got[:, 2] - want[:, 2]).max(), 0.0
    if n_obj:
        g = np.stack([o.ox[0], o.oy[0], o.otheta[0], o.ovx[0], o.ovy[0], o.ow[0]], -1).astype(np.float64)
        w = np.array(ref['objects'])
        pos, ang = max(pos, np.abs(g[:, :2] - w[:, :2]).max()), max(ang, np.abs(g[:, 2] - w[:, 2]).max())
        vel = np.abs(g[:, 3:] - w[:, 3:]).max()
    return float(pos), float(ang), float(vel)
