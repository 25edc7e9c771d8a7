"""Seeded synthetic scenes shared by the parity tests and bench.py."""
import numpy as np

from oracle import oracle as O

W, H = 2.0, 1.5          # kilobots_env.py:19


def gaussian_spawn(E, N, sigma, seed, mean=(0.0, 0.0), random_theta=True):
    """YamlKilobotsEnv._init_kilobots spawn rule, yaml_kilobots_env.py:346-352."""
    rng = np.random.RandomState(seed)
    xy = rng.normal(scale=sigma, size=(E, N, 2)) + np.asarray(mean)
    lo = np.array([-W / 2, -H / 2]) + 0.02
    hi = np.array([W / 2, H / 2]) - 0.02
    xy = np.minimum(np.maximum(xy, lo), hi)
    th = rng.uniform(-np.pi, np.pi, size=(E, N)) if random_theta else np.zeros((E, N))
    return xy, th


def lattice_spawn(E, N, seed, pitch=0.045, jitter=0.004):
    """cfg3: bots on a jittered square lattice (no initial overlap), SURVEY.md 8d item 3."""
    rng = np.random.RandomState(seed)
    side = int(np.ceil(np.sqrt(N)))
    idx = np.arange(N)
    gx = (idx % side - (side - 1) / 2.0) * pitch
    gy = (idx // side - (side - 1) / 2.0) * pitch
    xy = np.stack([gx, gy], -1)[None] + rng.uniform(-jitter, jitter, size=(E, N, 2))
    th = rng.uniform(-np.pi, np.pi, size=(E, N))
    return xy, th


def random_actions(E, N, seed):
    """U([0, 0.01] x [-pi/2, pi/2]): SimpleVelocityControlKilobot.action_space, kilobot.py:216-218."""
    rng = np.random.RandomState(seed)
    a = rng.uniform([0.0, -np.pi / 2], [0.01, np.pi / 2], size=(E, N, 2))
    return a.astype(np.float32)


def world(xy_m, th):
    """Poses in metres and radians as KilobotSim.set_poses_m stores them: (x, y, th) float32, world units."""
    xy = np.asarray(xy_m, np.float64) * 25.0
    return xy[..., 0].astype(np.float32), xy[..., 1].astype(np.float32), np.asarray(th, np.float32)


def put_numpy(sim, name, val):
    getattr(sim, name)[...] = val


# ---- ids and cases of the parametrised scene tables --------------------------------------------------------------------
def scene_id(s):
    return s.name


def sleep_cases(table):
    """(scene, allow_sleep) of a table whose scenes may be marked sleep_only"""
    return [(s, sl) for s in table for sl in (0, 1) if sl or not s.sleep_only]


def case_id(c):
    return '%s-%s' % (c[0].name, 'sleep' if c[1] else 'nosleep')


CFG4_OBJECTS = np.array([[0.5, 0.35], [-0.5, 0.35], [-0.5, -0.35], [0.5, -0.35]])
CFG4_RADIUS = 0.075


def cfg4_actions(xy, th_unused, seed):
    """cfg4: half the bots (even ids) head for the nearest object at full speed, the rest act randomly.
    Velocity-control actions cannot set the heading directly, so the chasers get omega towards the target."""
    E, N, _ = xy.shape
    a = random_actions(E, N, seed)
    return a


def toward_objects_theta(xy):
    """Initial headings: even bots face their nearest cfg4 object, odd bots keep a seeded random heading."""
    d = xy[:, :, None, :] - CFG4_OBJECTS[None, None]
    k = np.argmin((d ** 2).sum(-1), axis=-1)
    tgt = CFG4_OBJECTS[k]
    return np.arctan2(tgt[..., 1] - xy[..., 1], tgt[..., 0] - xy[..., 0])


# ---- boxes / polygons with friction and rotation -----------------------------------------------
def shape_kw(shapes):
    """shapes: list of ('box', w, h) | ('circle', r) | ('poly', [(x, y), ...]) -> config keywords (metres)."""
    kw = dict(obj_shape=[], obj_verts=[], obj_radius=[], obj_nverts=[])
    for sh in shapes:
        if sh[0] == 'box':
            kw['obj_shape'].append(O.SHAPE_BOX); kw['obj_verts'].append([[sh[1] / 2 * 25.0, sh[2] / 2 * 25.0]]); kw['obj_radius'].append(0.0); kw['obj_nverts'].append(4)
        elif sh[0] == 'circle':
            kw['obj_shape'].append(O.SHAPE_CIRCLE); kw['obj_verts'].append([[0.0, 0.0]]); kw['obj_radius'].append(sh[1]); kw['obj_nverts'].append(0)
        else:
            kw['obj_shape'].append(O.SHAPE_POLYGON); kw['obj_verts'].append([[v[0] * 25.0, v[1] * 25.0] for v in sh[1]]); kw['obj_radius'].append(0.0); kw['obj_nverts'].append(len(sh[1]))
    return kw


TRIANGLE_M = [(0.05, -0.05), (0.05, 0.10), (-0.10, -0.05)]      # metres: body.py:265-275 scaled to 0.15 x 0.15, recentred
MIXED_SHAPES = [('box', 0.15, 0.15), ('circle', 0.06), ('box', 0.2, 0.1), ('poly', TRIANGLE_M)]


def reference_polygon_fixtures(raw, width=0.15, height=0.15):
    """Sub-polygons of a lib.body.Polygon subclass -> hull-ordered fixtures in world units (what the env uploads)."""
    from gym_kilobots_amd.lib.body import _hull_order
    v = np.array(raw, dtype=np.float64)
    v = v / (v.max((0, 1)) - v.min((0, 1))) * np.array((width, height))
    cen, area = np.zeros(2), 0.0
    for vs in v:
        a = 0.5 * abs(np.dot(vs[:, 0], np.roll(vs[:, 1], 1)) - np.dot(vs[:, 1], np.roll(vs[:, 0], 1)))
        area += a
        cen += vs.mean(0) * a
    v = v - cen / area
    return [[list(q) for q in _hull_order([tuple(x) for x in vs * 25.0])] for vs in v]


LFORM = [[(-0.05, 0.0), (0.1, 0.0), (0.1, 0.3), (-0.05, 0.3)], [(0.1, 0.0), (0.1, -0.15), (-0.2, -0.15), (-0.2, 0.0)]]
CFORM = [[(0.09, 0.15), (0.09, -0.15), (-0.01, -0.15), (-0.01, 0.15)], [(-0.01, -0.15), (-0.11, -0.15), (-0.11, -0.08), (-0.01, -0.05)],
         [(-0.01, 0.15), (-0.11, 0.15), (-0.11, 0.08), (-0.01, 0.05)]]


def compound_kw():
    """Objects: 0 = LForm (2 fixtures), 1 = disc, 2 = CForm (3 fixtures), 3 = box: 7 fixtures, not adjacent per body."""
    lf, cf = reference_polygon_fixtures(LFORM), reference_polygon_fixtures(CFORM)
    fixtures = [(2, lf[0], 0), (0, None, 1), (2, cf[0], 2), (2, lf[1], 0), (2, cf[1], 2), (1, [[0.05 * 25.0, 0.1 * 25.0]], 3), (2, cf[2], 2)]
    kw = dict(num_objects=4, num_fixtures=len(fixtures), obj_fixture_body=[f[2] for f in fixtures] + [0],
              obj_shape=[f[0] for f in fixtures], obj_nverts=[0 if f[1] is None else len(f[1]) for f in fixtures],
              obj_radius=[0.05 if f[0] == 0 else 0.0 for f in fixtures],
              obj_verts=[[[0.0, 0.0]] if f[1] is None else f[1] for f in fixtures])
    return kw
