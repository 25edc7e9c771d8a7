"""The scenes of the randomised parity sweep (tests/test_parity_fuzz_gpu.py), drawn without a sim: bot counts, drive laws,
light models, object shapes with random fixture-to-body maps, spawn densities, solver paths, arena sizes, sleeping phases,
mixed laws, sensing, few warm-start slots.  Every stream is drawn in the order the sweep has always drawn it, so seed s is the
scene it always was.  Shared with tests/test_limits_cpu.py, which walks the same scenes on the oracle and the limits model."""
import os
from types import SimpleNamespace

import numpy as np

from oracle import oracle as O
from tests import limits_model as LM
from tests import scenes
from tests.gpu_common import OBJ_FIELDS

DEFAULT_SEEDS = 40
LAUNCHES = 12


def seeds():
    return list(range(int(os.environ.get('KB_FUZZ_SEEDS', str(DEFAULT_SEEDS)))))


def _random_objects(rng):
    """Random bodies: circles, boxes, triangles and two-/three-part compounds; fixtures shuffled across bodies."""
    from gym_kilobots_amd.lib.body import _hull_order
    nobj = int(rng.integers(1, 5))
    fixtures = []                      # (shape, verts or None, radius, body)
    for b in range(nobj):
        kind = rng.choice(['circle', 'box', 'tri', 'two', 'three']) if len(fixtures) <= 5 else rng.choice(['circle', 'box'])
        if kind == 'circle':
            fixtures.append((O.SHAPE_CIRCLE, None, float(rng.uniform(0.03, 0.07)), b))
        elif kind == 'box':
            fixtures.append((O.SHAPE_BOX, [[float(rng.uniform(0.03, 0.09)) * 25.0, float(rng.uniform(0.03, 0.09)) * 25.0]], 0.0, b))
        elif kind == 'tri':
            fixtures.append((O.SHAPE_POLYGON, [[x * 25.0, y * 25.0] for x, y in scenes.TRIANGLE_M], 0.0, b))
        else:
            parts = 2 if kind == 'two' else 3
            w, h = float(rng.uniform(0.04, 0.07)), float(rng.uniform(0.02, 0.04))
            for k in range(parts):     # a row of boxes glued together (as explicit quads)
                cx = (k - (parts - 1) / 2) * 2 * w
                quad = [(cx - w, -h), (cx + w, -h), (cx + w, h * (1 + 0.5 * k)), (cx - w, h)]
                fixtures.append((O.SHAPE_POLYGON, [list(q) for q in _hull_order([(x * 25.0, y * 25.0) for x, y in quad])], 0.0, b))
    fixtures = fixtures[:8]
    nobj = len({f[3] for f in fixtures})
    remap = {b: i for i, b in enumerate(sorted({f[3] for f in fixtures}))}
    order = rng.permutation(len(fixtures))
    fixtures = [fixtures[i] for i in order]
    # a circle must be alone on its body: guaranteed by construction
    pad = 8 - len(fixtures)
    kw = dict(num_objects=nobj, num_fixtures=len(fixtures), obj_fixture_body=[remap[f[3]] for f in fixtures] + [0] * pad,
              obj_shape=[f[0] for f in fixtures], obj_nverts=[0 if f[1] is None else len(f[1]) for f in fixtures],
              obj_radius=[f[2] for f in fixtures], obj_verts=[[[0.0, 0.0]] if f[1] is None else f[1] for f in fixtures])
    return nobj, kw


def scene(seed):
    """Everything test_random_scene needs of seed `seed`:
      E, N, mode, light, kw     arguments of tests.gpu_common.make_pair / oracle.default_config
      xy, th                    kilobot poses
      objs, oth, ovx            object poses and their velocity at the start (None without objects)
      light_x                   None without a light
      laws, motors              mixed drive laws: bot_mode and (motor_l, motor_r); else None
      motors_off                sleeping scenes under a motor law: mask of the kilobots whose motors are switched off; else None
      launches                  [(n_substeps, actions or None, light_action or None)] of the twelve launches
      fields                    what is compared bit for bit after every launch"""
    rng = np.random.default_rng(1000 + seed)
    N = int(rng.choice([1, 2, 7, 16, 33, 64, 100, 128, 200, 256, 300]))
    if os.environ.get('KB_FUZZ_BIG'):
        N = int(rng.choice([512, 700, 1000, 1024, 1024]))
    E = int(rng.integers(1, 5))
    mode = int(rng.choice([O.DRIVE_VELOCITY, O.DRIVE_VELOCITY, O.DRIVE_ACCEL, O.DRIVE_MOTORS, O.DRIVE_SIMPLE_PHOTOTAXIS, O.DRIVE_PHOTOTAXIS]))
    light = O.LIGHT_NONE
    if mode in (O.DRIVE_SIMPLE_PHOTOTAXIS, O.DRIVE_PHOTOTAXIS) or rng.random() < 0.3:
        light = int(rng.choice([O.LIGHT_CIRCULAR, O.LIGHT_GRADIENT, O.LIGHT_MOMENTUM]))
    kw = dict(solver_mode=int(rng.choice([0, 0, 0, 1, 2, 3, 4])), toi_walls=int(rng.random() < 0.8))
    # arena size (grid dimensions, LDS footprint, workgroups per CU) and iteration counts: from their own stream, so that
    # the scenes of the seeds keep their layout
    rng2 = np.random.default_rng(777000 + seed)
    W, H = 2.0, 1.5
    if rng2.random() < 0.5:
        W, H = [(1.0, 0.8), (1.2, 0.9), (3.0, 2.0), (0.6, 0.6), (2.0, 0.5)][int(rng2.integers(0, 5))]
        kw.update(world_width=W, world_height=H)
    if rng2.random() < 0.3:
        kw.update(vel_iters=int(rng2.choice([6, 3, 1])), pos_iters=int(rng2.choice([4, 2, 1, 0])))
    # sleeping (b2World doSleep): in 40 % of the scenes, with phases in which kilobots rest so that islands fall asleep and
    # are woken again (drawn last from the second stream: the older scenes keep their layout)
    sleeping = rng2.random() < 0.4
    if sleeping:
        kw.update(allow_sleep=1)
    # mixed drive laws (KB_DRIVE_MIXED): in a quarter of the scenes, every kilobot its own law and the
    # classes' densities (drawn after everything else from the second stream)
    mixed = rng2.random() < 0.25
    if mixed:
        mode = O.DRIVE_MIXED
        kw.update(mode_density=[2.0, 2.0, 1.0, 1.0, 1.0])
    sx, sy = W / 2.0, H / 1.5
    # fused neighbour sensing (kb_config.sense_radius): in half the scenes, one cell to more than two cells of reach scaled to the
    # arena; from a third stream of its own (the scenes keep their layout, and sensing does not change the step)
    rng3 = np.random.default_rng(555000 + seed)
    sense_radius = 0.0
    if rng3.random() < 0.5:
        sense_radius = float(rng3.choice([0.04, 0.07, 0.15])) * min(sx, sy)
        kw.update(sense_radius=sense_radius)
    # few warm-start slots (kb_config.ws_slots): in a third of the scenes, from a fourth stream of its own.  A kilobot with more
    # contacts than slots sets status bit 1 on both sides and ends nothing: the oracle says which entries are kept
    # (tests/overflow_scenes.py), so these scenes are compared for all twelve steps
    rng4 = np.random.default_rng(333000 + seed)
    if rng4.random() < 1.0 / 3.0:
        kw.update(ws_slots=int(rng4.choice([1, 2, 4, 8])))
    with_objects = rng.random() < 0.6
    nobj = 0
    if with_objects:
        nobj, okw = _random_objects(rng)
        kw.update(okw)
    sigma = float(rng.choice([0.03, 0.08, 0.2, 0.5]))
    if os.environ.get('KB_FUZZ_BIG'):
        sigma = float(rng.choice([0.12, 0.2, 0.3, 0.5]))
    xy = np.clip(rng.normal(scale=sigma, size=(E, N, 2)) + rng.uniform(-0.5, 0.5, (E, 1, 2)) * [sx, sy],
                 [-W / 2 + 0.03, -H / 2 + 0.03], [W / 2 - 0.03, H / 2 - 0.03])
    th = rng.uniform(-np.pi, np.pi, (E, N))
    s = SimpleNamespace(seed=seed, E=E, N=N, mode=mode, light=light, kw=kw, xy=xy, th=th, nobj=nobj, objs=None, oth=None, ovx=None,
                        light_x=None, laws=None, motors=None, motors_off=None, sleeping=sleeping)
    if nobj:
        s.objs = rng.uniform([-0.8, -0.55], [0.8, 0.55], (E, nobj, 2)) * [sx, sy]
        s.oth = rng.uniform(-np.pi, np.pi, (E, nobj))
        s.ovx = rng.uniform(-6, 6, (E, nobj)).astype(np.float32)
    if light != O.LIGHT_NONE:
        # (one light: OracleSim keeps light_x as [E])
        s.light_x = (rng.uniform(-0.5, 0.5, (E,)) * min(sx, sy)).astype(np.float32)
    if mixed:
        s.laws = rng2.integers(0, 5, (E, N)).astype(np.uint8)
        ml, mr = rng2.integers(0, 256, (E, N)).astype(np.uint8), rng2.integers(0, 256, (E, N)).astype(np.uint8)
        ml[rng2.random((E, N)) < 0.3] = 0
        s.motors = (ml, mr)
    s.fields = ('x', 'y', 'theta') + (OBJ_FIELDS[3:] if nobj else ())
    if sleeping:
        s.fields += ('sleep_time',) + (('osleep',) if nobj else ())
        if mode in (O.DRIVE_MOTORS, O.DRIVE_PHOTOTAXIS):      # a third of the kilobots has its motors off
            s.motors_off = rng2.random((E, N)) < 0.35
    if sense_radius > 0.0:
        s.fields += ('nbr_count',)
    la_dim = {O.LIGHT_NONE: 0, O.LIGHT_GRADIENT: 1}.get(light, 2)
    s.launches = []
    for k in range(LAUNCHES):
        la = None if la_dim == 0 or k % 3 == 2 else rng.uniform(-0.02, 0.02, (E, la_dim)).astype(np.float32)
        n_sub = int(rng.choice([1, 1, 3, 10]))
        a = None
        if mode in (O.DRIVE_VELOCITY, O.DRIVE_ACCEL, O.DRIVE_MIXED):
            a = scenes.random_actions(E, N, seed=5000 + 31 * seed + k)
            if sleeping:      # resting phases: everybody for a few steps, then a random half
                if k % 6 in (1, 2, 3):
                    a[...] = 0.0
                elif k % 6 == 4:
                    a[rng2.random((E, N)) < 0.5] = 0.0
                if mode == O.DRIVE_ACCEL and k % 6 in (1, 2, 3):
                    a[..., 0] = -0.005        # decelerate to a halt (the command is clamped at 0)
                    a[..., 1] = 0.0
        s.launches.append((n_sub, a, la))
    s.what = 'seed %d (N=%d E=%d mode=%d light=%d objects=%d %s)' % (seed, N, E, mode, light, nobj, kw.get('solver_mode'))
    return s



def oracle_sim(s, **changes):
    kw = dict(s.kw)
    kw.setdefault('allow_sleep', 0)
    kw.update(changes)
    return O.OracleSim(O.default_config(s.E, s.N, s.mode, s.light, **kw))


def start(s, osim):
    """The start state of scene s into an OracleSim.  -> the names of the buffers written besides the poses of kilobots and
    objects: a device sim takes the poses the same way and these buffers from the oracle's arrays"""
    osim.set_poses_m(s.xy, s.th)
    written = []
    if s.nobj:
        osim.set_objects_m(s.objs, s.oth)
        osim.ovx[...] = s.ovx
        written += ['ovx']
    if s.light_x is not None:
        osim.light_x[...] = s.light_x
        written += ['light_x']
    if s.laws is not None:
        osim.bot_mode[...] = s.laws
        osim.motor_l[...], osim.motor_r[...] = s.motors
        written += ['bot_mode', 'motor_l', 'motor_r']
    if s.motors_off is not None:
        osim.motor_l[s.motors_off] = 0
        osim.motor_r[s.motors_off] = 0
        written += ['motor_l', 'motor_r']
    return written


# ---- the limits model along a scene ---------------------------------------------------------------------------------------
def handle_limits(s, lib, nat):
    """(limits, shape) of the handle kb_create makes of scene s (tests/limits_model.py) -- no GPU needed"""
    kw = dict(s.kw)
    kw.setdefault('allow_sleep', 0)
    return LM.handle_limits(lib, nat, kw, s.N, s.mode, s.light)


def model_launch(osim, lim, shape, n_substeps, light_action):
    """Take the oracle through one launch substep by substep (the same bits as the fused call: tests/test_limits_cpu.py) with
    the model in front of every substep.  -> (must [E], may [E]): the status bits 2 and 3 that the device must have raised by
    the end of this launch, and those it may raise -- `must`, a level table that overflows only if the cooperative sweep
    runs where the counts do not say whether it does, and everything where the model itself could not see all contacts."""
    E = osim.cfg.num_envs
    must, may = np.zeros(E, np.int32), np.zeros(E, np.int32)
    for _ in range(n_substeps):
        for e, q in enumerate(LM.evaluate(osim, light_action)):
            over = LM.exceeded(q, lim, LM.level_sweep(q, lim, shape, osim.cfg.solver_mode))
            must[e] |= LM.expected_bits(over)
            may[e] |= LM.expected_bits(over) | (LM.BIT_STAGING if 'depth?' in over else 0)
            if q.hidden:
                may[e] |= LM.BIT_STAGING | LM.BIT_CANDIDATES
        osim.step(1, light_action=light_action)
    return must, may


def walk(s, lim, shape):
    """Scene s on the oracle and the model alone: (launches compared before the scene ends, why it ends: None | 'capacity' |
    'limit'), as test_random_scene ends it on a device that flags exactly what it must"""
    osim = oracle_sim(s)
    start(s, osim)
    for k, (n_sub, a, la) in enumerate(s.launches):
        if a is not None:
            osim.set_actions(a)
        must, may = model_launch(osim, lim, shape, n_sub, la)
        if (osim.status & 1).any():
            return k, 'capacity'
        if may.any():
            return k, 'limit'
    return len(s.launches), None
