"""GPU parity: the HIP world step (through the C ABI) against the CPU oracle on the same seeded
inputs, plus size-independent properties at full benchmark size.

The step is specified operation-by-operation in fp32 and both sides are compiled with
-ffp-contract=off, so the bar here is BIT-EXACT poses, commands and warm-start impulses; the
float32 tolerance the north star allows (1e-6 m absolute on positions) is asserted only where the
comparison is against float64 golden data from the reference."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import scenes
from tests.gpu_common import OBJ_FIELDS, assert_same, assert_ws_same, cpu, dev, make_pair

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [O.DRIVE_VELOCITY, O.DRIVE_ACCEL, O.DRIVE_MOTORS])
def test_contact_free_drive_modes(mode):
    E, N = 3, 64
    xy, th = scenes.lattice_spawn(E, N, seed=1, pitch=0.08)
    osim, gsim = make_pair(E, N, mode, xy=xy, th=th)
    rng = np.random.RandomState(5)
    if mode == O.DRIVE_MOTORS:
        ml = rng.randint(0, 256, size=(E, N)).astype(np.uint8)
        mr = rng.randint(0, 256, size=(E, N)).astype(np.uint8)
        ml[0, :8] = 0
        mr[0, 8:16] = 0
        ml[0, 16:20] = 0
        mr[0, 16:20] = 0
        osim.motor_l[...] = ml
        osim.motor_r[...] = mr
        gsim.motor_l.copy_(dev(ml))
        gsim.motor_r.copy_(dev(mr))
    for k in range(4):
        if mode != O.DRIVE_MOTORS:
            scale = 1.0 if mode == O.DRIVE_VELOCITY else 2.0
            a = (scenes.random_actions(E, N, seed=10 + k) * scale - (0 if mode == O.DRIVE_VELOCITY else 0.004)).astype(np.float32)
            osim.set_actions(a)
            gsim.set_actions(dev(a))
        osim.step(5)
        gsim.step(5)
        fields = ('x', 'y', 'theta', 'cmd_vx', 'cmd_vy', 'cmd_w') + (('v', 'w') if mode != O.DRIVE_MOTORS else ())
        assert_same(osim, gsim, 'mode %d step %d' % (mode, k), fields)
    assert osim.count_contacts(0) == (0, 0)
    assert int(cpu(gsim.status).max()) == 0


def test_golden_vectors_through_the_c_abi(golden):
    """Reference-generated vectors (tools/gen_golden.py) checked on the HIP path itself."""
    from gym_kilobots_amd.sim import KilobotSim
    cases = golden['a3_velocity']['cases']
    n = len(cases)
    g = KilobotSim(1, n, O.DRIVE_VELOCITY, debug_outputs=True)
    xy = np.stack([np.linspace(-0.8, 0.8, n), np.zeros(n)], -1)[None]
    g.set_poses_m(xy, np.array([[c['theta'] for c in cases]]))
    g.step(1, actions=dev(np.array([[c['action'] for c in cases]], np.float32)))
    torch.cuda.synchronize()
    got = np.stack([cpu(g.cmd_vx)[0], cpu(g.cmd_vy)[0], cpu(g.cmd_w)[0]], -1)
    np.testing.assert_allclose(got, [c['vel'] for c in cases], rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(np.stack([cpu(g.v)[0], cpu(g.w)[0]], -1), [c['clamped'] for c in cases], rtol=1e-6, atol=1e-9)
    cases = golden['a2_motor']['cases']
    n = len(cases)
    g = KilobotSim(1, n, O.DRIVE_MOTORS, debug_outputs=True)
    xy = np.stack([np.linspace(-0.9, 0.9, n), np.zeros(n)], -1)[None]
    g.set_poses_m(xy, np.array([[c['theta'] for c in cases]]))
    g.motor_l.copy_(dev(np.array([[c['left'] for c in cases]], np.uint8)))
    g.motor_r.copy_(dev(np.array([[c['right'] for c in cases]], np.uint8)))
    g.step(1)
    torch.cuda.synchronize()
    got = np.stack([cpu(g.cmd_vx)[0], cpu(g.cmd_vy)[0], cpu(g.cmd_w)[0]], -1)
    np.testing.assert_allclose(got, [c['vel'] for c in cases], rtol=2e-5, atol=2e-7)


def run_velocity_scene(E, N, xy, th, steps, substeps=10, seed=100, check_every=1, **kw):
    osim, gsim = make_pair(E, N, O.DRIVE_VELOCITY, xy=xy, th=th, **kw)
    for k in range(steps):
        a = scenes.random_actions(E, N, seed=seed + k)
        osim.set_actions(a)
        osim.step(substeps)
        gsim.step(substeps, actions=dev(a))
        if (k + 1) % check_every == 0 or k == steps - 1:
            assert_same(osim, gsim, 'env.step %d' % k, ('x', 'y', 'theta', 'v', 'w'))
            assert_ws_same(osim, gsim, 'env.step %d' % k)
    return osim, gsim


def test_cfg1_one_env_16_bots_gaussian_spawn():
    """BASELINE config 1: 1 env x 16 kilobots, random motor commands, 100 env.steps."""
    xy, th = scenes.gaussian_spawn(1, 16, sigma=0.1, seed=0, random_theta=False)
    osim, gsim = run_velocity_scene(1, 16, xy, th, steps=100, check_every=10)
    assert int(cpu(gsim.status).max()) == 0


def test_cfg2_slice_64_envs_64_bots():
    """BASELINE config 2 (256 x 64) on a 64-env slice: envs are independent, see the shard test."""
    xy, th = scenes.gaussian_spawn(64, 64, sigma=0.15, seed=2)
    osim, gsim = run_velocity_scene(64, 64, xy, th, steps=12, check_every=3)
    nb = sum(osim.count_contacts(e)[0] for e in range(64))
    assert nb > 0, 'scene is supposed to be in contact'
    assert int(cpu(gsim.status).max()) == 0 and int(osim.status.max()) == 0


def test_dense_cluster_256_bots():
    xy, th = scenes.gaussian_spawn(6, 256, sigma=0.2, seed=3)
    osim, gsim = run_velocity_scene(6, 256, xy, th, steps=4)
    assert sum(osim.count_contacts(e)[0] for e in range(6)) > 200


def test_1024_bots_lattice_then_crowding():
    """1024 bots packed on a lattice slightly tighter than 2r (every neighbour pair in contact from the
    start) and driven towards the arena centre: one big island, ~2000 contacts per env."""
    E, N = 2, 1024
    xy, th = scenes.lattice_spawn(E, N, seed=4, pitch=0.0325, jitter=0.0004)
    th = np.arctan2(-xy[..., 1], -xy[..., 0])       # face the arena centre
    osim, gsim = make_pair(E, N, O.DRIVE_VELOCITY, xy=xy, th=th)
    a = np.zeros((E, N, 2), np.float32)
    a[..., 0] = 0.01
    for k in range(3):
        osim.set_actions(a)
        osim.step(10)
        gsim.step(10, actions=dev(a))
        assert_same(osim, gsim, 'crowd step %d' % k)
        assert_ws_same(osim, gsim, 'crowd step %d' % k)
    assert osim.count_contacts(0)[0] > 1500
    assert int(cpu(gsim.status).max()) == 0


def test_walls_and_corners():
    E, N = 1, 32
    rng = np.random.RandomState(7)
    xy = np.zeros((E, N, 2))
    th = np.zeros((E, N))
    # 8 bots per wall, heading into it, plus corner huggers
    for i in range(8):
        xy[0, i] = (-0.97, -0.6 + 0.15 * i); th[0, i] = np.pi + rng.uniform(-0.5, 0.5)
        xy[0, 8 + i] = (0.97, -0.6 + 0.15 * i); th[0, 8 + i] = rng.uniform(-0.5, 0.5)
        xy[0, 16 + i] = (-0.8 + 0.2 * i, -0.72); th[0, 16 + i] = -np.pi / 2 + rng.uniform(-0.5, 0.5)
        xy[0, 24 + i] = (-0.8 + 0.2 * i, 0.72); th[0, 24 + i] = np.pi / 2 + rng.uniform(-0.5, 0.5)
    xy[0, 0] = (-0.975, -0.725); th[0, 0] = -3 * np.pi / 4
    xy[0, 15] = (0.975, 0.725); th[0, 15] = np.pi / 4
    osim, gsim = make_pair(E, N, O.DRIVE_VELOCITY, xy=xy, th=th)
    a = np.zeros((E, N, 2), np.float32)
    a[..., 0] = 0.01
    for k in range(6):
        osim.set_actions(a)
        osim.step(10)
        gsim.step(10, actions=dev(a))
        assert_same(osim, gsim, 'wall step %d' % k)
        assert_ws_same(osim, gsim, 'wall step %d' % k)
    assert osim.count_contacts(0)[1] >= 30
    # nobody left the arena: centre stays >= r + polygonRadius - 3 slop inside (world units / 25)
    p = osim.poses_m()[0]
    lim = 0.0165 + (0.01 - 0.015) / 25 - 1e-6
    assert (np.abs(p[:, 0]) <= 1.0 - lim).all() and (np.abs(p[:, 1]) <= 0.75 - lim).all()


@pytest.mark.parametrize('toi', [0, 1])
def test_continuous_step_against_walls(toi):
    """b2World::SolveTOI restated for the walls: pivoting kilobots (2.5 mm per substep) and a pushed disc hit the
    walls at every phase; with toi_walls=1 nobody ends a substep deeper than the TOI target."""
    E, N = 2, 48
    rng = np.random.RandomState(29)
    xy = np.zeros((E, N, 2))
    for e in range(E):
        xy[e, :12] = np.stack([0.975 - rng.uniform(0, 0.004, 12), np.linspace(-0.6, 0.6, 12)], -1)
        xy[e, 12:24] = np.stack([-0.975 + rng.uniform(0, 0.004, 12), np.linspace(-0.6, 0.6, 12)], -1)
        xy[e, 24:36] = np.stack([np.linspace(-0.8, 0.8, 12), 0.725 - rng.uniform(0, 0.004, 12)], -1)
        xy[e, 36:48] = np.stack([np.linspace(-0.8, 0.8, 12), -0.725 + rng.uniform(0, 0.004, 12)], -1)
    th = rng.uniform(-np.pi, np.pi, size=(E, N))
    objs = np.tile(np.array([[0.9, 0.2], [-0.55, -0.655]])[None], (E, 1, 1))
    osim, gsim = make_pair(E, N, O.DRIVE_MOTORS, xy=xy, th=th, objects=objs, toi_walls=toi)
    ml = np.where(rng.rand(E, N) < 0.5, 255, 0).astype(np.uint8)
    mr = (255 - ml).astype(np.uint8)
    osim.motor_l[...], osim.motor_r[...] = ml, mr
    gsim.motor_l.copy_(dev(ml))
    gsim.motor_r.copy_(dev(mr))
    deepest = 1.0
    for k in range(40):
        osim.step(1)
        gsim.step(1)
        assert_same(osim, gsim, 'toi=%d substep %d' % (toi, k), OBJ_FIELDS)
        p = osim.poses_m()
        deepest = min(deepest, (1.0 - np.abs(p[..., 0])).min(), (0.75 - np.abs(p[..., 1])).min())
    assert int(cpu(gsim.status).max()) == 0
    if toi:
        assert deepest > 0.0165 - 0.005 / 25 - 0.25 * 0.005 / 25 - 1e-6     # TOI target - tolerance
    else:
        assert deepest < 0.0165 - 0.0008                                     # discrete step alone tunnels ~1-2 mm


def _deepest_vertex_margin(osim, verts_w):
    """smallest wall distance (world units) of any vertex of single-fixture polygon objects with body-frame vertices verts_w"""
    om = osim.objects_m()
    c, s_ = np.cos(om[..., 2])[..., None], np.sin(om[..., 2])[..., None]
    vx = om[..., 0:1] * 25.0 + c * verts_w[:, 0] - s_ * verts_w[:, 1]
    vy = om[..., 1:2] * 25.0 + s_ * verts_w[:, 0] + c * verts_w[:, 1]
    return min((25.0 - np.abs(vx)).min(), (18.75 - np.abs(vy)).min())


@pytest.mark.parametrize('toi', [0, 1])
def test_continuous_step_of_polygon_objects(toi):
    """b2World::SolveTOI for polygon bodies: spinning boxes thrown at the walls and into the corners at 0.5 - 2 units per
    substep.  The TOI sub-solve runs on the manifold constraints (friction, block solver); bit-exact against the oracle
    in single-substep and fused launches, and with toi_walls=1 no vertex ends a substep beyond the TOI target."""
    E, N, M = 6, 4, 4
    xy = np.tile(np.array([[0.0, 0.0], [0.05, 0.0], [0.0, 0.05], [0.05, 0.05]])[None], (E, 1, 1))
    shapes = [('box', 0.15, 0.15)] * M
    rng = np.random.default_rng(41)
    objs = np.tile(np.array([[0.6, 0.3], [-0.6, 0.35], [0.5, -0.4], [-0.55, -0.35]])[None], (E, 1, 1)) + rng.uniform(-0.05, 0.05, (E, M, 2))
    oth = rng.uniform(-3.0, 3.0, (E, M))
    sp = rng.uniform(5.0, 20.0, (E, M)).astype(np.float32)
    dirs = rng.uniform(-0.6, 0.6, (E, M)) + np.array([0.0, np.pi, -0.7, np.pi + 0.7])[None]     # outwards, the last two into corners
    v0, vy0 = (sp * np.cos(dirs)).astype(np.float32), (sp * np.sin(dirs)).astype(np.float32)
    w0 = rng.uniform(-6.0, 6.0, (E, M)).astype(np.float32)
    hw = 0.075 * 25.0
    verts = np.array([[-hw, -hw], [hw, -hw], [hw, hw], [-hw, hw]])
    pairs = []
    for fused in (False, True):
        osim, gsim = make_pair(E, N, xy=xy, th=np.zeros((E, N)), num_objects=M, toi_walls=toi, **scenes.shape_kw(shapes))
        osim.set_objects_m(objs, oth)
        gsim.set_objects_m(objs, oth)
        osim.ovx[...] = v0; osim.ovy[...] = vy0; osim.ow[...] = w0
        gsim.ovx.copy_(dev(v0)); gsim.ovy.copy_(dev(vy0)); gsim.ow.copy_(dev(w0))
        pairs.append((osim, gsim))
    (o1, g1), (o2, g2) = pairs
    deepest = 1e9
    for k in range(30):
        o1.step(1)
        g1.step(1)
        assert_same(o1, g1, 'object toi=%d substep %d' % (toi, k), OBJ_FIELDS)
        deepest = min(deepest, _deepest_vertex_margin(o1, verts))
    o2.step(30)
    g2.step(30)
    assert_same(o2, g2, 'object toi=%d fused' % toi, OBJ_FIELDS)
    assert_same(o1, g2, 'object toi=%d fused == single' % toi, OBJ_FIELDS)
    assert int(cpu(g1.status).max()) == 0
    if toi:
        assert deepest > 0.005 - 0.00125 - 1e-4          # TOI target - tolerance (core polygon to wall line)
    else:
        assert deepest < -0.1                            # the discrete step alone lets corners through the wall


@pytest.mark.parametrize('mode', [O.DRIVE_SIMPLE_PHOTOTAXIS, O.DRIVE_PHOTOTAXIS])
def test_light_driven_modes(mode):
    E, N = 8, 48
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.12, seed=9)
    bounds = dict(light_lo=(-1.1, -0.825), light_hi=(1.1, 0.825), light_radius=0.4)
    osim, gsim = make_pair(E, N, mode, O.LIGHT_CIRCULAR, xy=xy, th=th, **bounds)
    rng = np.random.RandomState(11)
    l0 = rng.uniform(-0.3, 0.3, size=(E, 2)).astype(np.float32)
    osim.light_x[...] = l0[:, 0]
    osim.light_y[...] = l0[:, 1]
    gsim.light_x.copy_(dev(l0[:, 0]))
    gsim.light_y.copy_(dev(l0[:, 1]))
    fields = ('x', 'y', 'theta', 'light_x', 'light_y', 'light_value', 'light_gx', 'light_gy', 'cmd_vx', 'cmd_vy', 'cmd_w')
    if mode == O.DRIVE_PHOTOTAXIS:
        fields += ('motor_l', 'motor_r', 'pt_threshold', 'pt_update', 'pt_nochange', 'pt_dir')
    for k in range(8):
        la = rng.uniform(-0.02, 0.02, size=(E, 2)).astype(np.float32)
        if k == 3:
            osim.step(10)
            gsim.step(10)               # action None: light not stepped (kilobots_env.py:171)
        else:
            osim.step(10, light_action=la)
            gsim.step(10, light_action=dev(la))
        assert_same(osim, gsim, 'light mode %d step %d' % (mode, k), fields)
    assert int(cpu(gsim.status).max()) == 0


@pytest.mark.parametrize('light', ['gradient', 'momentum', 'composite'])
def test_other_light_models(light):
    """GradientLight, MomentumLight, CompositeLight evaluated and stepped on the device."""
    E, N = 6, 40
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.15, seed=19)
    rng = np.random.RandomState(23)
    b = dict(light_lo=(-1.1, -0.825), light_hi=(1.1, 0.825))
    if light == 'gradient':
        kw, lt, adim = {}, O.LIGHT_GRADIENT, 1
    elif light == 'momentum':
        kw, lt, adim = dict(light_radius=0.5, light_max_velocity=0.01, **b), O.LIGHT_MOMENTUM, 2
    else:
        kw = dict(light_count=3, light_kind=[O.LIGHT_CIRCULAR, O.LIGHT_MOMENTUM, O.LIGHT_CIRCULAR],
                  lightc_radius=[0.3, 0.4, 0.25], lightc_max_velocity=[np.inf, 0.008, np.inf],
                  lightc_lo=[b['light_lo']] * 3 + [(0, 0)], lightc_hi=[b['light_hi']] * 3 + [(0, 0)])
        lt, adim = O.LIGHT_COMPOSITE, 6
    for mode in (O.DRIVE_SIMPLE_PHOTOTAXIS, O.DRIVE_PHOTOTAXIS):
        osim, gsim = make_pair(E, N, mode, lt, xy=xy, th=th, **kw)
        l0 = rng.uniform(-0.4, 0.4, size=osim.light_x.shape).astype(np.float32)
        l1 = rng.uniform(-0.4, 0.4, size=osim.light_x.shape).astype(np.float32)
        v0 = rng.uniform(-0.005, 0.005, size=osim.light_x.shape).astype(np.float32)
        for name, val in (('light_x', l0), ('light_y', l1), ('light_vx', v0), ('light_vy', -v0)):
            getattr(osim, name)[...] = val
            getattr(gsim, name).copy_(dev(val))
        fields = ('x', 'y', 'theta', 'light_x', 'light_y', 'light_vx', 'light_vy', 'light_value', 'light_gx', 'light_gy')
        for k in range(5):
            la = rng.uniform(-7.0 if light == 'gradient' else -0.02, 7.0 if light == 'gradient' else 0.02,
                             size=(E, adim)).astype(np.float32)
            if k == 2:
                osim.step(10)
                gsim.step(10)
            else:
                osim.step(10, light_action=la)
                gsim.step(10, light_action=dev(la))
            assert_same(osim, gsim, '%s light mode %d step %d' % (light, mode, k), fields)
        assert int(cpu(gsim.status).max()) == 0


def test_reset_step_resolves_overlaps_without_drive():
    """KilobotsEnv.reset: one world.Step with zero velocities pushes overlapping bodies apart
    (kilobots_env.py:156-157); heavy initial overlap like kilobots_test_envs.py:53-82."""
    E, N = 4, 15
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.02, seed=13, random_theta=False)
    xy[:, 5] = xy[:, 0]                    # exactly coincident pair (kilobots_test_envs.py:53,63)
    osim, gsim = make_pair(E, N, O.DRIVE_VELOCITY, xy=xy, th=th, ws_slots=16)
    d0 = np.linalg.norm(xy[:, :, None] - xy[:, None, :], axis=-1)
    for k in range(5):
        osim.step(1, flags=O.STEP_NO_DRIVE)
        gsim.step(1, flags=O.STEP_NO_DRIVE)
        assert_same(osim, gsim, 'resolve %d' % k)
        assert_ws_same(osim, gsim, 'resolve %d' % k)
    p = osim.poses_m()[..., :2]
    d1 = np.linalg.norm(p[:, :, None] - p[:, None, :], axis=-1)
    iu = np.triu_indices(N, 1)
    assert d1[:, iu[0], iu[1]].mean() > d0[:, iu[0], iu[1]].mean()


@pytest.mark.parametrize('mode', [1, 2, 3, 4])
def test_every_solver_path_gives_the_same_bits(mode):
    """The kernel picks between a register-resident solver, per-wave list sweeps, whole-workgroup sweeps
    and LDS / global contact staging by scene density; every path must reproduce the oracle exactly."""
    E, N = 6, 256
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.2, seed=3)
    osim, gsim = run_velocity_scene(E, N, xy, th, steps=3, solver_mode=mode)
    assert int(cpu(gsim.status).max()) == 0
    xy, th = scenes.lattice_spawn(2, 1024, seed=4, pitch=0.0325, jitter=0.0004)
    run_velocity_scene(2, 1024, xy, th, steps=2, solver_mode=mode)


def test_moderate_density_uses_the_register_solver_and_matches():
    """cfg3-like steady state (~500 contacts per env, small islands): the automatic path."""
    E, N = 4, 1024
    xy, th = scenes.lattice_spawn(E, N, seed=1000)
    osim, gsim = make_pair(E, N, O.DRIVE_VELOCITY, xy=xy, th=th)
    for k in range(60):
        a = scenes.random_actions(E, N, seed=2000 + k % 8)
        osim.set_actions(a)
        osim.step(1)
        gsim.step(1, actions=dev(a))
        if k % 10 == 9:
            assert_same(osim, gsim, 'substep %d' % k)
            assert_ws_same(osim, gsim, 'substep %d' % k)
    nb = osim.count_contacts(0)[0]
    assert 200 < nb < 1000
    assert int(cpu(gsim.status).max()) == 0


# ---- pushable objects (BASELINE config 4) ---------------------------------------------------------
@pytest.mark.parametrize('mode', [0, 1, 2, 3, 4])
def test_objects_pushed_by_a_crowd(mode):
    """4 discs of radius 0.075 m at the cfg4 positions inside a 256-bot crowd: kilobot-object, object-wall
    contacts, warm-start tables; every solver path."""
    E, N = 3, 256
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.3, seed=61)
    th = scenes.toward_objects_theta(xy)
    objs = np.tile(scenes.CFG4_OBJECTS[None], (E, 1, 1))
    osim, gsim = make_pair(E, N, xy=xy, th=th, objects=objs, solver_mode=mode)
    a = np.zeros((E, N, 2), np.float32)
    a[..., 0] = 0.01
    for k in range(5):
        osim.set_actions(a)
        osim.step(10)
        gsim.step(10, actions=dev(a))
        assert_same(osim, gsim, 'objects mode %d step %d' % (mode, k), OBJ_FIELDS)
        assert_ws_same(osim, gsim, 'objects mode %d step %d' % (mode, k))
    assert osim.count_contacts(0, True)[2] > 3
    assert int(cpu(gsim.status).max()) == 0
    assert np.abs(osim.objects_m()[..., :2] - objs).max() > 1e-4        # the discs were actually pushed


@pytest.mark.parametrize('drive', [O.DRIVE_VELOCITY, O.DRIVE_ACCEL, O.DRIVE_MOTORS, O.DRIVE_SIMPLE_PHOTOTAXIS, O.DRIVE_PHOTOTAXIS])
@pytest.mark.parametrize('N', [40, 200])
def test_disc_objects_in_every_drive_mode(drive, N):
    """Scenes whose objects are all discs run the instantiations without the polygon contact code (one per drive law, as a
    one-wave 256-VGPR kernel at 40 kilobots and as a regular one at 200): bit-exact against the oracle, discs pushed,
    thrown at a wall and at each other."""
    E = 3
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.25, seed=140 + N)
    th = scenes.toward_objects_theta(xy)
    objs = np.tile(scenes.CFG4_OBJECTS[None, :3], (E, 1, 1))
    light = O.LIGHT_CIRCULAR if drive in (O.DRIVE_SIMPLE_PHOTOTAXIS, O.DRIVE_PHOTOTAXIS) else O.LIGHT_NONE
    kw = dict(light_lo=(-1.1, -0.825), light_hi=(1.1, 0.825), light_radius=0.6) if light != O.LIGHT_NONE else {}
    osim, gsim = make_pair(E, N, drive, light, xy=xy, th=th, objects=objs, **kw)
    v0 = np.tile(np.array([8.0, -5.0, 0.0], np.float32)[None], (E, 1))
    osim.ovx[...] = v0
    gsim.ovx.copy_(dev(v0))
    rng = np.random.RandomState(3)
    if drive == O.DRIVE_MOTORS:
        ml = np.where(rng.rand(E, N) < 0.5, 255, 0).astype(np.uint8)
        osim.motor_l[...], osim.motor_r[...] = ml, 255 - ml
        gsim.motor_l.copy_(dev(ml)); gsim.motor_r.copy_(dev((255 - ml).astype(np.uint8)))
    for k in range(5):
        kws_o, kws_g = {}, {}
        if light != O.LIGHT_NONE:
            la = rng.uniform(-0.02, 0.02, size=(E, 2)).astype(np.float32)
            kws_o, kws_g = dict(light_action=la), dict(light_action=dev(la))
        if drive in (O.DRIVE_VELOCITY, O.DRIVE_ACCEL):
            a = scenes.random_actions(E, N, seed=150 + k)
            osim.set_actions(a)
            kws_g['actions'] = dev(a)
        osim.step(10, **kws_o)
        gsim.step(10, **kws_g)
        assert_same(osim, gsim, 'discs drive %d N %d step %d' % (drive, N, k), OBJ_FIELDS)
        assert_ws_same(osim, gsim, 'discs drive %d N %d step %d' % (drive, N, k))
    assert int(cpu(gsim.status).max()) == 0
    assert np.abs(osim.objects_m()[..., :2] - objs).max() > 1e-3


def test_object_object_and_object_wall_contacts():
    E, N = 2, 6
    xy = np.tile(np.array([[0.55, 0.02 * (i - 2.5)] for i in range(6)])[None], (E, 1, 1))
    xy[1, :, 1] += 0.01
    objs = np.tile(np.array([[0.66, 0.0], [0.83, 0.0]])[None], (E, 1, 1))
    osim, gsim = make_pair(E, N, xy=xy, th=np.zeros((E, N)), objects=objs)
    a = np.zeros((E, N, 2), np.float32)
    a[..., 0] = 0.01
    for k in range(45):
        osim.set_actions(a)
        osim.step(10)
        gsim.step(10, actions=dev(a))
        if k % 5 == 4:
            assert_same(osim, gsim, 'two discs step %d' % k, OBJ_FIELDS)
    assert osim.objects_m()[0, 1, 0] > 0.92 and int(cpu(gsim.status).max()) == 0


@pytest.mark.parametrize('mode', [0, 1, 2, 3])
def test_cfg4_slice_1024_bots_4_objects(mode):
    """BASELINE config 4 geometry on 2 envs (lattice of 1024 bots overlapping four discs at reset); velocity control,
    no light, 1024 kilobots, discs only: the disc-only fixed-size instantiation, in every solver path.  One disc is
    thrown at the wall (continuous step of an object) and one at its neighbour (object-object manifold)."""
    E, N = 2, 1024
    xy, th = scenes.lattice_spawn(E, N, seed=71)
    th = scenes.toward_objects_theta(xy)
    objs = np.tile(scenes.CFG4_OBJECTS[None], (E, 1, 1))
    osim, gsim = make_pair(E, N, xy=xy, th=th, objects=objs, solver_mode=mode)
    v0 = np.zeros((E, objs.shape[1]), np.float32)
    v0[:, 0], v0[:, 1] = 9.0, -4.0
    osim.ovx[...] = v0
    gsim.ovx.copy_(dev(v0))
    osim.step(1, flags=O.STEP_NO_DRIVE)
    gsim.step(1, flags=O.STEP_NO_DRIVE)             # reset(): step to resolve the initial overlaps
    assert_same(osim, gsim, 'cfg4 resolve', OBJ_FIELDS)
    for k in range(3):
        a = scenes.random_actions(E, N, seed=80 + k)
        a[:, ::2, 0] = 0.01
        a[:, ::2, 1] = 0.0
        osim.set_actions(a)
        osim.step(10)
        gsim.step(10, actions=dev(a))
        assert_same(osim, gsim, 'cfg4 mode %d step %d' % (mode, k), OBJ_FIELDS)
        assert_ws_same(osim, gsim, 'cfg4 mode %d step %d' % (mode, k))
    assert osim.count_contacts(0, True)[2] > 10
    assert int(cpu(gsim.status).max()) == 0


# ---- boxes / polygons with friction and rotation (shapes in tests/scenes.py) -----------------------
@pytest.mark.parametrize('mode', [0, 1, 2, 3, 4])
def test_boxes_pushed_by_a_crowd(mode):
    """Two boxes, a disc and a triangle at the cfg4 positions inside a 256-bot crowd: kilobot-polygon contacts with
    lever arms, object rotation, every solver path."""
    E, N = 3, 256
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.3, seed=62)
    th = scenes.toward_objects_theta(xy)
    objs = np.tile(scenes.CFG4_OBJECTS[None], (E, 1, 1))
    oth = np.tile(np.array([0.3, 0.0, -0.7, 1.1])[None], (E, 1))
    osim, gsim = make_pair(E, N, xy=xy, th=th, solver_mode=mode, num_objects=4, **scenes.shape_kw(scenes.MIXED_SHAPES))
    osim.set_objects_m(objs, oth)
    gsim.set_objects_m(objs, oth)
    a = np.zeros((E, N, 2), np.float32)
    a[..., 0] = 0.01
    for k in range(6):
        osim.set_actions(a)
        osim.step(10)
        gsim.step(10, actions=dev(a))
        assert_same(osim, gsim, 'boxes mode %d step %d' % (mode, k), OBJ_FIELDS)
        assert_ws_same(osim, gsim, 'boxes mode %d step %d' % (mode, k))
    assert osim.count_contacts(0, True)[2] > 3
    assert int(cpu(gsim.status).max()) == 0
    assert np.abs(osim.objects_m()[..., 2] - oth).max() > 1e-4           # something was turned


def test_box_wall_box_box_and_disc_manifolds():
    """Objects shoved into each other and into the walls by their own initial velocity: two-point manifolds, block
    solver, friction, feature-id warm starting; bit-exact every substep."""
    E, N = 4, 4
    xy = np.tile(np.array([[-0.9, 0.7], [-0.85, 0.7], [-0.8, 0.7], [-0.75, 0.7]])[None], (E, 1, 1))
    shapes = [('box', 0.15, 0.15), ('box', 0.2, 0.1), ('circle', 0.05), ('poly', scenes.TRIANGLE_M), ('box', 0.1, 0.1)]
    osim, gsim = make_pair(E, N, xy=xy, th=np.zeros((E, N)), num_objects=5, **scenes.shape_kw(shapes))
    rng = np.random.default_rng(9)
    objs = np.tile(np.array([[0.7, 0.0], [0.45, 0.02], [0.3, -0.05], [0.6, 0.3], [0.8, -0.5]])[None], (E, 1, 1))
    objs = objs + rng.uniform(-0.01, 0.01, objs.shape)
    oth = rng.uniform(-1.0, 1.0, (E, 5))
    oth[0] = 0.0                                                         # env 0: everything axis-aligned
    osim.set_objects_m(objs, oth)
    gsim.set_objects_m(objs, oth)
    v0 = np.zeros((E, 5), np.float32)
    v0[:] = [6.0, 9.0, 12.0, 5.0, 7.0]
    vy0 = np.tile(np.array([0.0, 0.2, 0.5, -3.0, -6.0], np.float32)[None], (E, 1))
    osim.ovx[...] = v0; osim.ovy[...] = vy0
    gsim.ovx.copy_(dev(v0)); gsim.ovy.copy_(dev(vy0))
    two_point = False
    for k in range(60):
        osim.step(1)
        gsim.step(1)
        assert_same(osim, gsim, 'manifolds substep %d' % k, OBJ_FIELDS)
        two_point |= bool((osim.ows_acc[..., 3] >= 0).any())
    assert two_point, 'no two-point manifold occurred'
    assert int(cpu(gsim.status).max()) == 0
    osim.step(40)
    gsim.step(40)                                                         # fused launch, resting contacts
    assert_same(osim, gsim, 'manifolds fused', OBJ_FIELDS)


@pytest.mark.parametrize('mode', [0, 1, 2, 3])
def test_multi_fixture_bodies_in_a_crowd(mode):
    """LForm / CForm bodies (several convex fixtures, centre of mass off the body origin) among 256 kilobots."""
    E, N = 3, 256
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.3, seed=63)
    th = scenes.toward_objects_theta(xy)
    objs = np.tile(scenes.CFG4_OBJECTS[None], (E, 1, 1))
    oth = np.tile(np.array([0.4, 0.0, -1.2, 0.8])[None], (E, 1))
    osim, gsim = make_pair(E, N, xy=xy, th=th, solver_mode=mode, **scenes.compound_kw())
    osim.set_objects_m(objs, oth)
    gsim.set_objects_m(objs, oth)
    a = np.zeros((E, N, 2), np.float32)
    a[..., 0] = 0.01
    for k in range(6):
        osim.set_actions(a)
        osim.step(10)
        gsim.step(10, actions=dev(a))
        assert_same(osim, gsim, 'compound mode %d step %d' % (mode, k), OBJ_FIELDS)
        assert_ws_same(osim, gsim, 'compound mode %d step %d' % (mode, k))
    assert osim.count_contacts(0, True)[2] > 3
    assert int(cpu(gsim.status).max()) == 0
    assert np.abs(osim.objects_m()[..., 2] - oth).max() > 1e-4


def test_multi_fixture_bodies_collide_with_walls_and_each_other():
    E, N = 4, 2
    xy = np.tile(np.array([[-0.9, 0.7], [-0.85, 0.7]])[None], (E, 1, 1))
    osim, gsim = make_pair(E, N, xy=xy, th=np.zeros((E, N)), **scenes.compound_kw())
    rng = np.random.default_rng(19)
    objs = np.tile(np.array([[0.55, 0.0], [0.3, 0.05], [0.8, -0.1], [0.75, 0.35]])[None], (E, 1, 1)) + rng.uniform(-0.01, 0.01, (E, 4, 2))
    oth = rng.uniform(-1.5, 1.5, (E, 4))
    osim.set_objects_m(objs, oth)
    gsim.set_objects_m(objs, oth)
    v0 = np.tile(np.array([7.0, 12.0, 3.0, 2.0], np.float32)[None], (E, 1))
    vy0 = np.tile(np.array([0.5, -0.5, 1.0, -4.0], np.float32)[None], (E, 1))
    w0 = np.tile(np.array([0.5, 0.0, -0.3, 0.2], np.float32)[None], (E, 1))
    osim.ovx[...] = v0; osim.ovy[...] = vy0; osim.ow[...] = w0
    gsim.ovx.copy_(dev(v0)); gsim.ovy.copy_(dev(vy0)); gsim.ow.copy_(dev(w0))
    touched = False
    for k in range(70):
        osim.step(1)
        gsim.step(1)
        assert_same(osim, gsim, 'compound manifolds substep %d' % k, OBJ_FIELDS)
        touched |= bool((osim.ows_acc[..., 0] >= 0).any())
    assert touched and int(cpu(gsim.status).max()) == 0
    osim.step(30)
    gsim.step(30)
    assert_same(osim, gsim, 'compound manifolds fused', OBJ_FIELDS)


def test_eight_objects_every_candidate_index():
    """8 objects = 60 manifold candidates (28 pairs + 32 object-wall): the objects fly apart into all four walls and
    into each other, so candidates with high indices (mask bits >= 31) are active."""
    E, N = 2, 2
    xy = np.tile(np.array([[0.0, 0.0], [0.04, 0.0]])[None], (E, 1, 1))
    shapes = [('box', 0.1, 0.1), ('circle', 0.04), ('box', 0.12, 0.06), ('circle', 0.05),
              ('poly', scenes.TRIANGLE_M), ('box', 0.08, 0.08), ('circle', 0.03), ('box', 0.1, 0.05)]
    osim, gsim = make_pair(E, N, xy=xy, th=np.zeros((E, N)), num_objects=8, **scenes.shape_kw(shapes))
    ang = np.linspace(0, 2 * np.pi, 8, endpoint=False) + 0.2
    objs = np.tile(np.stack([0.45 * np.cos(ang), 0.4 * np.sin(ang)], -1)[None], (E, 1, 1))
    objs[1] *= 0.97
    oth = np.tile(np.linspace(-1, 1, 8)[None], (E, 1))
    osim.set_objects_m(objs, oth)
    gsim.set_objects_m(objs, oth)
    v = (14.0 * np.stack([np.cos(ang), np.sin(ang)], -1)).astype(np.float32)
    osim.ovx[...] = v[:, 0]; osim.ovy[...] = v[:, 1]
    gsim.ovx.copy_(dev(np.tile(v[None, :, 0], (E, 1)))); gsim.ovy.copy_(dev(np.tile(v[None, :, 1], (E, 1))))
    seen = set()
    for k in range(80):
        osim.step(1)
        gsim.step(1)
        assert_same(osim, gsim, 'eight objects substep %d' % k, OBJ_FIELDS)
        seen |= {(int(o), int(c)) for _, o, c in np.argwhere(osim.ows_acc[..., 0] >= 0)}
    walls = {c for _, c in seen if c >= 8}
    assert len(walls) == 4, 'all four walls should have been hit: %s' % sorted(seen)
    assert any(o >= 6 and c >= 8 for o, c in seen), 'no high candidate index was active: %s' % sorted(seen)
    assert int(cpu(gsim.status).max()) == 0


def test_1024_bots_with_boxes():
    E, N = 2, 1024
    xy, th = scenes.lattice_spawn(E, N, seed=72)
    th = scenes.toward_objects_theta(xy)
    objs = np.tile(scenes.CFG4_OBJECTS[None], (E, 1, 1))
    osim, gsim = make_pair(E, N, xy=xy, th=th, num_objects=4, **scenes.shape_kw(scenes.MIXED_SHAPES))
    osim.set_objects_m(objs)
    gsim.set_objects_m(objs)
    osim.step(1, flags=O.STEP_NO_DRIVE)
    gsim.step(1, flags=O.STEP_NO_DRIVE)
    assert_same(osim, gsim, 'boxes resolve', OBJ_FIELDS)
    for k in range(3):
        a = scenes.random_actions(E, N, seed=90 + k)
        a[:, ::2, 0] = 0.01
        a[:, ::2, 1] = 0.0
        osim.set_actions(a)
        osim.step(10)
        gsim.step(10, actions=dev(a))
        assert_same(osim, gsim, '1024 + boxes step %d' % k, OBJ_FIELDS)
        assert_ws_same(osim, gsim, '1024 + boxes step %d' % k)
    assert int(cpu(gsim.status).max()) == 0


# ---- size-independent properties on the HIP path --------------------------------------------------
def test_fused_launch_equals_single_substep_launches():
    """kb_step(10) == 10 x kb_step(1), bit for bit (state incl. warm-start cache is complete)."""
    from gym_kilobots_amd.sim import KilobotSim
    E, N = 256, 64
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.15, seed=21)
    a = dev(scenes.random_actions(E, N, seed=22))
    g1 = KilobotSim(E, N)
    g2 = KilobotSim(E, N)
    for g in (g1, g2):
        g.set_poses_m(xy, th)
        g.set_actions(a)
    for k in range(3):
        g1.step(10)
        for _ in range(10):
            g2.step(1)
    torch.cuda.synchronize()
    for f in ('x', 'y', 'theta', 'ws_cnt'):
        assert torch.equal(getattr(g1, f), getattr(g2, f)), f


def test_env_shard_equals_rows_of_unsharded_run():
    """Multi-GPU contract: shard k of the env axis == rows of the unsharded run."""
    from gym_kilobots_amd.sim import KilobotSim
    E, N = 64, 64
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.15, seed=31)
    a = scenes.random_actions(E, N, seed=32)
    full = KilobotSim(E, N)
    full.set_poses_m(xy, th)
    sl = slice(16, 32)
    part = KilobotSim(16, N)
    part.set_poses_m(xy[sl], th[sl])
    for k in range(3):
        full.step(10, actions=dev(a))
        part.step(10, actions=dev(a[sl]))
    torch.cuda.synchronize()
    for f in ('x', 'y', 'theta'):
        assert torch.equal(getattr(full, f)[sl], getattr(part, f)), f


def test_block_size_does_not_change_results():
    from gym_kilobots_amd.sim import KilobotSim
    E, N = 8, 256
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.2, seed=41)
    a = dev(scenes.random_actions(E, N, seed=42))
    outs = []
    for threads in (128, 256, 512):
        g = KilobotSim(E, N)
        g.block_threads = threads
        g.set_poses_m(xy, th)
        g.step(10, actions=a)
        g.step(10)
        torch.cuda.synchronize()
        outs.append((g.x.clone(), g.y.clone(), g.theta.clone()))
    for o in outs[1:]:
        for t0, t1 in zip(outs[0], o):
            assert torch.equal(t0, t1)


def test_cfg3_full_size_invariants_and_slice_parity():
    """BASELINE config 3 (4096 envs x 1024 bots): invariants on the whole batch, oracle parity on a slice."""
    from gym_kilobots_amd.sim import KilobotSim
    E, N = 4096, 1024
    xy1, th1 = scenes.lattice_spawn(8, N, seed=51)
    reps = E // 8
    xy, th = np.tile(xy1, (reps, 1, 1)), np.tile(th1, (reps, 1))
    a1 = scenes.random_actions(8, N, seed=52)
    g = KilobotSim(E, N)
    g.set_poses_m(xy, th)
    a = dev(np.tile(a1, (reps, 1, 1)))
    for k in range(2):
        g.step(10, actions=a)
    torch.cuda.synchronize()
    assert int(g.status.max().item()) == 0
    x, y, t = cpu(g.x), cpu(g.y), cpu(g.theta)
    assert np.isfinite(x).all() and np.isfinite(y).all() and np.isfinite(t).all()
    # replicas of the same 8 envs must be identical (no cross-env state, no nondeterminism)
    assert np.array_equal(x.reshape(reps, 8, N), np.broadcast_to(x[:8], (reps, 8, N)))
    assert np.array_equal(y.reshape(reps, 8, N), np.broadcast_to(y[:8], (reps, 8, N)))
    # and equal to the oracle on those 8 envs
    osim = O.OracleSim(O.default_config(8, N))
    osim.set_poses_m(xy1, th1)
    osim.set_actions(a1)
    osim.step(20, threads=8)
    assert np.array_equal(osim.x, x[:8]) and np.array_equal(osim.y, y[:8]) and np.array_equal(osim.theta, t[:8])
    # non-penetration: no pair closer than 2r - 3 slop - 1 substep of approach (2 * 0.0625 world units)
    px, py = x[:8].astype(np.float64), y[:8].astype(np.float64)
    for e in range(8):
        d = np.hypot(px[e][:, None] - px[e][None, :], py[e][:, None] - py[e][None, :])
        d[np.diag_indices(N)] = 10.0
        assert d.min() > 0.825 - 0.015 - 0.13


@pytest.mark.parametrize('variant', ['cfg3', 'cfg3_sleep', 'cfg4_discs', 'cfg4_boxes_sleep'])
def test_long_horizon_stays_bit_exact(variant):
    """Hundreds of substeps of the benchmark scenes (the settled regime the bench times: ~550 contacts per env, kilobots
    against the walls, continuous-step events, objects in the crowd), substep by substep launches and fused ones mixed:
    every bit of the state still equals the oracle at the end -- rare events do not drift apart."""
    N, E = 1024, 2
    xy, th = scenes.lattice_spawn(E, N, seed=77)
    kw, objects = {}, None
    if 'sleep' in variant:
        kw['allow_sleep'] = 1
    if variant.startswith('cfg4'):
        objects = np.tile(scenes.CFG4_OBJECTS[None], (E, 1, 1))
        if 'boxes' in variant:
            kw.update(obj_shape=[1] * 4 + [0] * 4, obj_nverts=[4] * 4 + [0] * 4,
                      obj_verts=[[[0.075 * 25.0, 0.075 * 25.0]] + [[0.0, 0.0]] * 3] * 4 + [[[0.0, 0.0]] * 4] * 4)
    osim, gsim = make_pair(E, N, xy=xy, th=th, objects=objects, **kw)
    steps = 240 if variant.startswith('cfg4') else 400
    k = 0
    while k < steps:
        a = scenes.random_actions(E, N, seed=9000 + k)
        if variant.startswith('cfg4'):
            a[:, ::2] = (0.01, 0.0)                 # every second kilobot rams ahead (the bench's cfg4 actions)
        if 'sleep' in variant and (k // 40) % 3 == 2:
            a[:, N // 3:] = 0.0                     # two thirds of the swarm rest for 40 substeps at a time
        n = 10 if (k // 10) % 4 == 3 else 1         # fused env.step launches in between
        osim.set_actions(a)
        osim.step(n, threads=2)
        gsim.step(n, actions=dev(a))
        k += n
    fields = ('x', 'y', 'theta') + (OBJ_FIELDS[3:] if objects is not None else ()) + (('sleep_time',) if 'sleep' in variant else ())
    assert_same(osim, gsim, variant, fields)
    assert_ws_same(osim, gsim, variant)
    assert int(cpu(gsim.status).max()) == 0 and int(osim.status.max()) == 0
    assert osim.ws_cnt.sum() / E > (600 if variant.startswith('cfg4') else 450)       # the settled, contact-rich regime
    if 'sleep' in variant:
        assert (osim.sleep_time < 0).any()


@pytest.mark.parametrize('N', [1024, 640])
def test_jammed_swarm_one_giant_island(N):
    """A swarm driven at a light jams into ONE island of more contacts than the LDS staging holds: the whole workgroup
    sweeps it key by key on records in the global scratch slice (tools/cluster_probe.py is the timing twin of this scene).
    Bit-exact against the oracle all the way into the jam."""
    E = 2
    xy, th = scenes.lattice_spawn(E, N, seed=77)
    osim, gsim = make_pair(E, N, O.DRIVE_SIMPLE_PHOTOTAXIS, O.LIGHT_CIRCULAR, xy=xy, th=th, light_radius=2.0)
    for s in (osim, gsim):
        s.light_x[...] = 0.0
        s.light_y[...] = 0.0
    for k in range(5):
        osim.step(50)
        gsim.step(50)
        assert_same(osim, gsim, 'jam, substep %d' % (50 * (k + 1)))
        assert_ws_same(osim, gsim)
    from tests import solver_regimes as SR
    counts = SR.counts(cpu(gsim.ws_cnt))
    band = (gsim.block_threads // SR.LANES, gsim.lds_staging_entries, gsim.contact_capacity)
    contacts = int(counts.min())
    # N = 1024: beyond 3 x the LDS staging (3 x 688), where the impulses stay in the global records; the oracle reaches 2260 there
    assert contacts > (2064 if N == 1024 else 600), 'contacts %s, regimes of the last substep %s at (waves, staged, capacity) = %s' \
        % (counts, SR.classify(cpu(gsim.ws_cnt), band), band)
    assert int(cpu(gsim.status).max()) == 0 and int(osim.status.max()) == 0
