"""The env-level API on the real HIP path: same scenes as tests/test_env_api_cpu.py, compared with
the oracle-backed stand-in env step by step (bit-exact poses)."""
import numpy as np
import pytest
import torch

from gym_kilobots_amd.envs import DirectControlKilobotsEnv, KilobotsEnv, BatchedKilobotsEnv
from gym_kilobots_amd.lib import SimpleVelocityControlKilobot, PhototaxisKilobot, CircularGradientLight
from tests.env_scenes import YAML_BOXES
from tests.oracle_backend import OracleBackend

pytestmark = pytest.mark.gpu


class CrowdEnv(DirectControlKilobotsEnv):
    def _configure_environment(self):
        rng = np.random.RandomState(0)
        for p in rng.normal(scale=0.05, size=(24, 2)):       # overlapping spawn, resolved by reset()
            self._add_kilobot(SimpleVelocityControlKilobot(self.world, position=p, orientation=rng.uniform(-3, 3),
                                                           velocity=[0.0, 0.0]))

    def get_reward(self, s, a, ns):
        return 0.


class LightEnv(KilobotsEnv):
    def _configure_environment(self):
        self._light = CircularGradientLight(position=np.array([0.2, 0.1]), radius=0.5)
        for i in range(15):
            self._add_kilobot(PhototaxisKilobot(self.world, position=(0.03 * (i % 5), 0.03 * (i // 5)), light=self._light))

    def get_reward(self, s, a, ns):
        return 1.


def test_direct_control_env_on_gpu_equals_oracle_env():
    g, o = CrowdEnv(), CrowdEnv(sim_factory=OracleBackend)
    og, oo = g.reset(), o.reset()
    assert np.array_equal(og['kilobots'], oo['kilobots'])
    rng = np.random.RandomState(1)
    for k in range(10):
        a = rng.uniform([0, -1.5], [0.01, 1.5], size=(24, 2))
        og, rg, dg, ig = g.step(a)
        oo, ro, do, io = o.step(a)
        assert np.array_equal(og['kilobots'], oo['kilobots']), k
    assert type(g.sim).__name__ == 'KilobotSim' and int(g.sim.status.max().item()) == 0
    kb = g.kilobots[3]
    np.testing.assert_allclose(kb.get_pose(), og['kilobots'][3], atol=1e-7)
    g.close()


def test_light_env_on_gpu_equals_oracle_env():
    g, o = LightEnv(), LightEnv(sim_factory=OracleBackend)
    g.reset(), o.reset()
    rng = np.random.RandomState(2)
    for k in range(8):
        a = rng.uniform(-0.02, 0.02, size=2)
        og, *_ = g.step(a)
        oo, *_ = o.step(a)
        assert np.array_equal(og['kilobots'], oo['kilobots']) and np.array_equal(og['light'], oo['light'])
    assert g.kilobots[0].get_motors() == o.kilobots[0].get_motors()


def test_batched_env_on_gpu():
    env = BatchedKilobotsEnv(32, 64, seed=5, reward_fn=lambda p, a, o: (o[..., :2] - p[..., :2]).norm(dim=-1).sum(-1))
    obs = env.reset()
    assert obs.is_cuda and obs.shape == (32, 64, 3)
    a = torch.rand(32, 64, 2, device=obs.device) * torch.tensor([0.01, 1.0], device=obs.device)
    for _ in range(3):
        obs, r, done, info = env.step(a)
    assert (r > 0).all() and torch.isfinite(obs).all()
    assert env.gather_episode_returns().shape == (32,)


def test_yaml_scene_with_boxes_on_gpu_equals_oracle_env():
    """The reference's object-pushing set-up (yaml_kilobots_env.py:216-242): a light drags the swarm into boxes; the
    env on the HIP path and the oracle-backed env see identical observations."""
    import yaml
    from gym_kilobots_amd.envs import YamlKilobotsEnv
    conf = yaml.load(YAML_BOXES, Loader=yaml.Loader)
    g = YamlKilobotsEnv(configuration=conf)
    o = YamlKilobotsEnv(configuration=conf, sim_factory=OracleBackend)
    np.random.seed(11)
    og = g.reset()
    np.random.seed(11)                                        # same random spawn for both
    oo = o.reset()
    assert np.array_equal(og['kilobots'], oo['kilobots']) and np.array_equal(og['objects'], oo['objects'])
    start = og['objects'].copy()
    for k in range(40):
        a = np.array([0.01, 0.002 * np.sin(0.3 * k)])
        og, *_ = g.step(a)
        oo, *_ = o.step(a)
        assert np.array_equal(og['kilobots'], oo['kilobots']), k
        assert np.array_equal(og['objects'], oo['objects']), k
    assert type(g.sim).__name__ == 'KilobotSim'
    assert int(g.sim.status.max().item()) == 0 and int(o.sim.status.max().item()) == 0     # ws_slots = 32 holds the dense spawn (and the env would have raised)
    assert np.abs(og['objects'] - start).max() > 1e-3          # the swarm moved something
    g.close()


@pytest.mark.parametrize('seed', [0, 1, 2, 3, 4, 5])
def test_random_yaml_scenes_on_gpu_equal_oracle_env(seed):
    """Random YAML documents (every shape string, every light type, random inits): env on the HIP path == oracle-backed env."""
    import yaml
    from gym_kilobots_amd.envs import YamlKilobotsEnv
    rng = np.random.RandomState(100 + seed)
    shapes = ['square', 'rect', 'corner_quad', 'triangle', 'circle', 'l_shape', 't_shape', 'c_shape']
    fixtures = {'square': 1, 'rect': 1, 'corner_quad': 1, 'triangle': 1, 'circle': 1, 'l_shape': 2, 't_shape': 2, 'c_shape': 3}
    objs, budget = [], 8
    for i in range(rng.randint(1, 5)):
        sh = shapes[rng.randint(len(shapes))]
        if fixtures[sh] > budget:
            continue
        budget -= fixtures[sh]
        w = float(rng.uniform(0.04, 0.07) if sh == 'circle' else rng.uniform(0.1, 0.2))
        init = 'random' if rng.rand() < 0.3 else [float(rng.uniform(-0.3, 0.3)), float(rng.uniform(-0.25, 0.25)), float(rng.uniform(-3, 3))]
        objs.append('    - !ObjectConf {idx: %d, shape: %s, width: %.3f, height: %.3f, init: %s, color: ~, symmetry: 1}'
                    % (i, sh, w, float(rng.uniform(0.1, 0.2)), init))
    kind = ['circular', 'momentum', 'linear', 'composite'][rng.randint(4)]
    if kind == 'linear':
        light = 'light: !LightConf {type: linear, init: %.3f}' % rng.uniform(-3, 3)
    elif kind == 'composite':
        light = ('light: !LightConf\n  type: composite\n  init: fixed\n  components:\n'
                 '    - !LightConf {type: circular, init: [-0.2, 0.0], radius: 0.3}\n'
                 '    - !LightConf {type: momentum, init: [0.2, 0.1], radius: 0.25}')
    else:
        light = 'light: !LightConf {type: %s, init: %s, radius: %.2f}' % (kind, 'random' if rng.rand() < 0.5 else '[0.1, -0.1]', rng.uniform(0.2, 0.5))
    doc = ('!EvalEnv\nwidth: 1.2\nheight: 0.9\nresolution: 500\nobjects:\n%s\n%s\n'
           'kilobots: !KilobotsConf {num: %d, mean: %s, std: %.3f}\n'
           % ('\n'.join(objs), light, rng.randint(5, 60), 'random' if rng.rand() < 0.3 else '[0.0, 0.0]', rng.uniform(0.05, 0.2)))
    conf = yaml.load(doc, Loader=yaml.Loader)
    g = YamlKilobotsEnv(configuration=conf)
    o = YamlKilobotsEnv(configuration=conf, sim_factory=OracleBackend)
    np.random.seed(7 + seed)
    og = g.reset()
    np.random.seed(7 + seed)
    oo = o.reset()
    adim = g.action_space.shape[0]
    for k in range(15):
        a = rng.uniform(-0.02, 0.02, adim) if kind != 'linear' else rng.uniform(-3, 3, adim)
        og, *_ = g.step(a)
        oo, *_ = o.step(a)
        for key in ('kilobots', 'objects', 'light'):
            assert np.array_equal(og[key], oo[key]), (seed, k, key, doc)
    g.close()
