"""KB_DRIVE_MIXED: any mix of the five drive laws in one env (the reference steps whatever is in `_kilobots`,
kilobots_env.py:183-184; its classes have different fixture densities, kilobot.py:25 / :214).

CPU: the oracle -- a contact-free mixed env follows the single-law sims kilobot by kilobot, masses differ by law in contacts.
GPU (-m gpu): the HIP path against the oracle bit for bit (contacts, objects, lights, sleeping), the env API."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import scenes

DENS = [2.0, 2.0, 1.0, 1.0, 1.0]          # SimpleVelocityControl / SimpleAccelerationControl 2.0 (kilobot.py:214), the others 1.0 (:25)


def _modes(E, N, seed):
    return np.random.RandomState(seed).randint(0, 5, size=(E, N)).astype(np.uint8)


def test_contact_free_mixed_env_follows_the_single_law_sims():
    E, N = 2, 10
    rng = np.random.RandomState(0)
    xy = np.tile(np.stack([np.linspace(-0.8, 0.8, N), np.linspace(-0.5, 0.5, N)], -1)[None], (E, 1, 1))
    th = rng.uniform(-3, 3, (E, N))
    modes = np.tile(np.arange(N, dtype=np.uint8) % 5, (E, 1))
    mix = O.OracleSim(O.default_config(E, N, O.DRIVE_MIXED, O.LIGHT_CIRCULAR, mode_density=DENS))
    mix.bot_mode[...] = modes
    a = rng.uniform([0, -1], [0.01, 1], (E, N, 2)).astype(np.float32)
    a[:, 1] = (0.004, 0.3)
    a[:, 6] = (-0.003, -0.2)
    singles = [O.OracleSim(O.default_config(E, N, m, O.LIGHT_CIRCULAR, bot_density=DENS[m])) for m in range(5)]
    for s in [mix] + singles:
        s.set_poses_m(xy, th)
        s.light_x[...] = 0.1
        s.light_y[...] = -0.05
    mix.set_actions(a)
    singles[0].set_actions(a)
    singles[1].set_actions(a)
    for k in range(30):
        la = rng.uniform(-0.01, 0.01, (E, 2)).astype(np.float32)
        for s in [mix] + singles:
            s.step(1, light_action=la)
    for b in range(N):
        s = singles[modes[0, b]]
        for f in ('x', 'y', 'theta'):
            assert np.array_equal(getattr(mix, f)[:, b], getattr(s, f)[:, b]), (b, f)
    assert np.abs(mix.x - xy[..., 0] * 25).max() > 0.05


def test_masses_differ_by_law_in_a_collision():
    # a velocity-control kilobot (density 2) meets a resting motor-law kilobot (density 1) head on: after the first touching
    # substep the normal velocities are shared in the ratio of the masses (inelastic contact, restitution 0)
    r = 0.0165
    mix = O.OracleSim(O.default_config(1, 2, O.DRIVE_MIXED, O.LIGHT_NONE, mode_density=DENS))
    mix.bot_mode[...] = [[0, 2]]
    mix.motor_l[...] = 0
    mix.motor_r[...] = 0
    mix.set_poses_m(np.array([[[0.0, 0.0], [2 * r + 0.002, 0.0]]]), np.zeros((1, 2)))
    a = np.zeros((1, 2, 2), np.float32)
    a[0, 0] = (0.01, 0.0)
    mix.set_actions(a)
    x0 = mix.x.copy()
    for _ in range(12):
        mix.step(1)
    d = mix.x - x0
    assert d[0, 1] > 0.0                      # the resting kilobot is pushed
    # its commanded velocity is 0, the pusher's 0.2315 units/s: with masses 2 : 1 the pair moves at 2/3 of the pusher's speed
    # while touching (each substep the drive law resets both velocities, the solver shares the momentum)
    same = O.OracleSim(O.default_config(1, 2, O.DRIVE_MIXED, O.LIGHT_NONE, mode_density=[1.0] * 5))
    same.bot_mode[...] = [[0, 2]]
    same.motor_l[...] = 0
    same.motor_r[...] = 0
    same.set_poses_m(np.array([[[0.0, 0.0], [2 * r + 0.002, 0.0]]]), np.zeros((1, 2)))
    same.set_actions(a)
    for _ in range(12):
        same.step(1)
    assert mix.x[0, 1] > same.x[0, 1] + 1e-3   # the heavier pusher shoves the pushed kilobot further than an equal one


# ---------------------------------------------------------------------------------------------------------------- GPU
def _pair(E, N, light=O.LIGHT_NONE, xy=None, th=None, objects=None, seed=0, **kw):
    from tests.gpu_common import make_pair, dev
    osim, gsim = make_pair(E, N, O.DRIVE_MIXED, light, xy=xy, th=th, objects=objects, mode_density=DENS, **kw)
    modes = _modes(E, N, seed)
    osim.bot_mode[...] = modes
    gsim.bot_mode.copy_(dev(modes))
    rng = np.random.RandomState(seed + 1)
    ml, mr = rng.randint(0, 256, (E, N)).astype(np.uint8), rng.randint(0, 256, (E, N)).astype(np.uint8)
    ml[rng.rand(E, N) < 0.3] = 0
    mr[rng.rand(E, N) < 0.3] = 0
    osim.motor_l[...] = ml
    osim.motor_r[...] = mr
    gsim.motor_l.copy_(dev(ml))
    gsim.motor_r.copy_(dev(mr))
    return osim, gsim


MIX_FIELDS = ('x', 'y', 'theta', 'v', 'w', 'cmd_vx', 'cmd_vy', 'cmd_w')


@pytest.mark.gpu
@pytest.mark.parametrize('N,light,sleep', [(16, O.LIGHT_NONE, 0), (64, O.LIGHT_CIRCULAR, 0), (100, O.LIGHT_MOMENTUM, 1), (128, O.LIGHT_GRADIENT, 1),
                                           (37, O.LIGHT_CIRCULAR, 1),
                                           # beyond 128 kilobots: the full workgroup at 256 VGPRs
                                           (129, O.LIGHT_NONE, 1), (300, O.LIGHT_CIRCULAR, 0), (1024, O.LIGHT_MOMENTUM, 1)])
def test_mixed_swarm_equals_oracle(N, light, sleep):
    from tests.gpu_common import assert_same, assert_ws_same, dev
    E = 3
    xy, th = scenes.gaussian_spawn(E, N, sigma=min(0.04 + 0.001 * N, 0.35), seed=N)
    kw = dict(light_max_velocity=0.05) if light == O.LIGHT_MOMENTUM else {}
    osim, gsim = _pair(E, N, light, xy=xy, th=th, seed=N, allow_sleep=sleep, **kw)
    if light != O.LIGHT_NONE:
        lx = np.random.RandomState(3).uniform(-0.3, 0.3, osim.light_x.shape).astype(np.float32)
        osim.light_x[...] = lx
        gsim.light_x.copy_(dev(lx))
    rng = np.random.RandomState(5)
    adim = {O.LIGHT_NONE: 0, O.LIGHT_GRADIENT: 1}.get(light, 2)
    for k in range(30):
        a = scenes.random_actions(E, N, seed=40 + k)
        if k % 7 in (3, 4):
            a[...] = 0.0
        la = None if adim == 0 or k % 3 == 2 else rng.uniform(-0.02, 0.02, (E, adim)).astype(np.float32)
        n = 10 if k % 5 == 4 else 1
        osim.set_actions(a)
        osim.step(n, light_action=la)
        gsim.step(n, actions=dev(a), light_action=None if la is None else dev(la))
        assert_same(osim, gsim, 'mixed N %d substep %d' % (N, k), MIX_FIELDS + (('sleep_time',) if sleep else ()))
    assert_ws_same(osim, gsim, 'mixed')
    assert osim.ws_cnt.sum() > 0
    assert int(gsim.status.max().item()) == 0 or N > 128      # (dense large spawns may flag slot overflows; still compared)


@pytest.mark.gpu
@pytest.mark.parametrize('solver_mode', [0, 1, 2, 3, 4])
def test_mixed_swarm_with_objects_on_every_solver_path(solver_mode):
    from tests.gpu_common import assert_same, dev, OBJ_FIELDS
    E, N = 2, 90
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.12, seed=8)
    objs = np.tile(np.array([[0.1, 0.05], [-0.15, -0.1]])[None], (E, 1, 1))
    kw = dict(obj_shape=[1, 0, 0, 0, 0, 0, 0, 0], obj_nverts=[4, 0, 0, 0, 0, 0, 0, 0],
              obj_verts=[[[0.075 * 25.0, 0.05 * 25.0]] + [[0.0, 0.0]] * 3] + [[[0.0, 0.0]] * 4] * 7, solver_mode=solver_mode)
    osim, gsim = _pair(E, N, O.LIGHT_CIRCULAR, xy=xy, th=th, objects=objs, seed=21, allow_sleep=1, **kw)
    for k in range(25):
        a = scenes.random_actions(E, N, seed=70 + k)
        osim.set_actions(a)
        osim.step(1)
        gsim.step(1, actions=dev(a))
        assert_same(osim, gsim, 'mixed objects mode %d substep %d' % (solver_mode, k), OBJ_FIELDS + ('sleep_time', 'osleep'))


@pytest.mark.gpu
def test_mixed_env_api_equals_oracle_env():
    """KilobotsEnv with kilobots of four classes (two drive families, two densities) and a box, on the HIP path and on the
    oracle-backed stand-in: bit-identical observations; set_action reaches the velocity kilobots only."""
    from gym_kilobots_amd.envs import KilobotsEnv
    from gym_kilobots_amd.lib import (SimpleVelocityControlKilobot, SimpleAccelerationControlKilobot, PhototaxisKilobot,
                                      SimplePhototaxisKilobot, CircularGradientLight, Quad)
    from tests.oracle_backend import OracleBackend

    class Zoo(KilobotsEnv):
        def _configure_environment(self):
            self._light = CircularGradientLight(position=np.array([0.15, 0.05]), radius=0.5)
            rng = np.random.RandomState(1)
            for i, p in enumerate(rng.normal(scale=0.06, size=(24, 2))):
                cls = (SimpleVelocityControlKilobot, PhototaxisKilobot, SimplePhototaxisKilobot, SimpleAccelerationControlKilobot)[i % 4]
                kw = dict(velocity=[0.004, 0.2]) if i % 4 in (0, 3) else dict(light=self._light)
                self._add_kilobot(cls(self.world, position=p, orientation=0.3 * i, **kw))
            self._add_object(Quad(width=0.1, height=0.08, position=(0.0, 0.22), world=self.world))

        def get_reward(self, *a):
            return 0.

    g, o = Zoo(), Zoo(sim_factory=OracleBackend)
    og, oo = g.reset(), o.reset()
    assert g.sim.drive_mode == 5 and np.array_equal(og['kilobots'], oo['kilobots'])
    rng = np.random.RandomState(2)
    for k in range(6):
        for env in (g, o):
            for kb in env.kilobots[::4]:
                kb.set_action(np.array([0.008, 0.4 - 0.1 * k]))
        a = rng.uniform(-0.02, 0.02, size=2)
        og, *_ = g.step(a)
        oo, *_ = o.step(a)
        assert np.array_equal(og['kilobots'], oo['kilobots']) and np.array_equal(og['objects'], oo['objects']), k
    assert np.abs(og['kilobots'][:, :2]).max() < 1.0
    g.close()
