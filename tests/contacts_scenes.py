"""The scenes of the kb_sense_contacts tests, for the CPU oracle and the device alike: S1 a crowd in a corner next to a disc,
S2 a Gaussian crowd of 300, S3 the lattice of 1024, S4b a dense heap on a large store.  Each is stepped once without drive
("resolve", one substep as kb_reset does), then driven for some 10-substep steps."""
import numpy as np

from tests import scenes

STEP_NO_DRIVE = 1


def s1():
    E, N = 2, 64
    rng = np.random.RandomState(5)
    xy = rng.normal(scale=0.05, size=(E, N, 2)) + np.array([-0.93, -0.68])
    xy = np.maximum(xy, np.array([-0.98, -0.73]))
    th = rng.uniform(-np.pi, np.pi, size=(E, N))
    a = np.zeros((E, N, 2), np.float32)
    a[..., 0] = 0.01
    objects = np.tile(np.array([[-0.80, -0.60]])[None], (E, 1, 1))
    return dict(E=E, N=N, xy=xy, th=th, actions=a, steps=3, objects=objects, kw=dict(num_objects=1, obj_radius=[0.075]))


def s2():
    E, N = 2, 300
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.12, seed=7)
    a = np.zeros((E, N, 2), np.float32)
    a[..., 0] = 0.01
    return dict(E=E, N=N, xy=xy, th=th, actions=a, steps=3, objects=None, kw={})


def s3():
    E, N = 2, 1024
    xy, th = scenes.lattice_spawn(E, N, seed=3)
    return dict(E=E, N=N, xy=xy, th=th, actions=scenes.random_actions(E, N, seed=1), steps=2, objects=None, kw={})


def s4b():
    E, N = 2, 200
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.05, seed=11)
    return dict(E=E, N=N, xy=xy, th=th, actions=None, steps=0, objects=None, kw=dict(contact_capacity=8192, ws_slots=64))


SCENES = dict(S1=s1, S2=s2, S3=s3, S4b=s4b)


def place(sim, sc):
    sim.set_poses_m(sc['xy'], sc['th'])
    if sc['objects'] is not None:
        sim.set_objects_m(sc['objects'])


def fixture_body(cfg):
    """The body of every fixture in the kb_config numbering."""
    if cfg.num_fixtures > 0:
        return [int(cfg.obj_fixture_body[f]) for f in range(cfg.num_fixtures)]
    return list(range(cfg.num_objects))


def oracle_run(sc, allow_sleep=0, **more):
    """The scene on the CPU oracle: (the sim after the resolve step -- a snapshot of its store --, the sim after the steps)."""
    from oracle import oracle as O
    kw = dict(sc['kw'], allow_sleep=allow_sleep, **more)
    o = O.OracleSim(O.default_config(sc['E'], sc['N'], **kw))
    place(o, sc)
    o.step(1, flags=STEP_NO_DRIVE)
    resolved = store(o)
    for _ in range(sc['steps']):
        o.set_actions(sc['actions'])
        o.step(10)
    return resolved, o


def store(o):
    """A copy of the oracle's store: (ws_cnt, ws_key, ws_acc, cap, status)."""
    return o.ws_cnt.copy(), o.ws_key.copy(), o.ws_acc.copy(), o.cap, o.status.copy()
