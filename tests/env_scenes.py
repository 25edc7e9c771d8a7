"""Env-level scenes that more than one module uses: a small direct-control env and the YAML box-pushing set-up, shared by the
env API tests on both backends (tests/test_env_api_cpu.py, tests/test_env_api_gpu.py), tests/test_render_cpu.py and
tools/debug_yaml_scene.py."""
import numpy as np

from gym_kilobots_amd.envs import DirectControlKilobotsEnv
from gym_kilobots_amd.lib import SimpleVelocityControlKilobot


class VelEnv(DirectControlKilobotsEnv):
    def _configure_environment(self):
        for i in range(6):
            self._add_kilobot(SimpleVelocityControlKilobot(self.world, position=(-0.25 + 0.1 * i, 0.05 * i),
                                                           orientation=0.3 * i, velocity=[0.005, 0.1]))

    def get_reward(self, state, action, new_state):
        return float(np.linalg.norm(new_state['kilobots'][:, :2] - state['kilobots'][:, :2]))


# the reference's object-pushing set-up (yaml_kilobots_env.py:216-242) as an !EvalEnv document
YAML_BOXES = """
!EvalEnv
width: 1.0
height: 0.8
resolution: 600
objects:
    - !ObjectConf {idx: 0, shape: square, width: 0.15, height: 0.15, init: [0.05, 0.0, 0.2], color: [10, 20, 255], symmetry: 4}
    - !ObjectConf {idx: 1, shape: corner_quad, width: 0.1, height: 0.2, init: [0.3, 0.1, -0.4], color: ~, symmetry: 1}
    - !ObjectConf {idx: 2, shape: triangle, width: 0.15, height: 0.15, init: [-0.2, -0.2, 1.0], color: ~, symmetry: 1}
    - !ObjectConf {idx: 3, shape: circle, width: 0.05, height: 0.05, init: [0.42, -0.3, 0.0], color: ~, symmetry: 1}
light: !LightConf {type: circular, init: [0.3, 0.0], radius: 0.4}
kilobots: !KilobotsConf {num: 40, mean: [-0.05, 0.0], std: 0.04}
"""
