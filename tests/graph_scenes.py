"""What is captured into a graph and replayed (tests/test_graph_replay_gpu.py): the table of the entries, their scenes and the
inputs of every replay.  Needs neither torch nor a device to import; what touches the device imports torch when it is called.

torch.cuda.graph is how a PyTorch user removes the launch cost the small configurations are bound by, and the library is
shaped for it: every entry is asynchronous on the current stream, masks, seeds and episode counters live on the device.  A
replay differs from the eager launch every other test makes: every scalar and pointer is frozen in the graph node at capture
(kb_params by value, kb_reset_params, kb_episode_init, the keep and spread arrays, the render style), outputs and temporaries
live in the graph's private pool, the kernarg segment the step kernels re-read per phase belongs to the node, and scratch and
status hold what the previous replay left.  Every row here is captured once and replayed R times next to a twin that makes
the same call eagerly; the two must agree bit for bit in every bound field and every output after every replay.

  SENSING    every row of residency_scenes.SENSORS (edges with a capacity, so that nothing is read back) and PATHS_BIG, on the
             residency scene at D = 5 envs; between replays both sims take BETWEEN substeps, so that every replay sees new poses
  STEP       one census row (tests/variant_census.py) per translation unit csrc/kb_inst_*.hip, each in the three FORMS
  RESETS     reset(seed) and reset_envs(mask, episode, objects, lights) on a case of tests/reset_envs_ref.py
  ENV        one BatchedKilobotsEnv.step with every device observation, a field, torch-only callbacks and auto-reset
  REFUSED    the public methods that must read the device: they raise ValueError inside a capture, before any launch

Shared by tests/test_graph_replay_cpu.py (the table against KilobotSim and the translation units, no replay vacuous on the
oracle, the capacity of the edge list) and tests/test_graph_replay_gpu.py."""
import collections
import glob
import os

import numpy as np

from oracle import oracle as O
from tests import residency_scenes as RS
from tests import scenes
from tests import variant_census as VC

D = RS.D
REPLAYS = 3
BETWEEN = 10                # substeps both sims take before every replay of a sensing row: an env.step of the reference


# ---- sensing ---------------------------------------------------------------------------------------------------------------
# the edges of the scene at the poses of replay 0, 1, 2 on the oracle (tests/test_graph_replay_cpu.py holds them against it), and
# the fixed length of the lists: no replay drops an edge
EDGES_NNZ = (16048, 16006, 15894)
EDGES_CAPACITY = 16384


def _edges(sim, out):
    e = sim.edges(RS.RADIUS, capacity=EDGES_CAPACITY, out=None if out is None else out[:3])
    return e.src, e.dst, e.rel, e.offsets, e.count, e.nnz


SENSING = [row if row.name != 'edges' else RS.Row('edges', 'edges', ('src', 'dst', 'rel', 'offsets', 'count', 'nnz'), _edges, ()) for row in RS.SENSORS] + [RS.PATHS_BIG]
SENSING_BY_NAME = {row.name: row for row in SENSING}
# the inputs of RS.inputs() a row reads: they are static tensors (RS.tiled) that every replay finds rewritten in place
SENSING_INPUTS = {'reduce-sum': ('messages',), 'reduce-min': ('messages',), 'hops': ('seeds',), 'field_step': ('field', 'amount', 'field_mask'),
                  'paths': ('source', 'blocked'), 'paths-128': ('source_big', 'blocked_big'), 'targets': ('points',), 'assign': ('points',),
                  'light_sense': ('light_action',)}


def sensing_inputs(n, k):
    """{name: array [D, ...]}: the inputs of replay k, the rows of RS.inputs() handed on by k + 1 envs.  The D rows of every
    input differ (tests/test_sensing_residency_cpu.py), so every env gets another row in every replay."""
    return {name: np.ascontiguousarray(np.roll(a, k + 1, axis=0)) for name, a in RS.inputs(n).items()}


def between_actions(n, k):
    """[D, n, 2]: the actions of the BETWEEN substeps before replay k"""
    return scenes.random_actions(D, n, seed=RS.ACTION_SEED + 1 + k)


def sensing_oracle(n):
    """The oracle at the poses of replay 0, 1, ... of a sensing row, one after the other (a generator: the same OracleSim,
    stepped on)."""
    o = RS.oracle_run(n)
    for k in range(REPLAYS):
        o.set_actions(between_actions(n, k))
        o.step(BETWEEN)
        yield o


# ---- step ------------------------------------------------------------------------------------------------------------------
# translation unit -> the position in kb_variants of the census row replayed for it
STEP_UNITS = collections.OrderedDict([
    ('d0', 160),            # the fixed-size kernel of 1024 kilobots
    ('d0_discs', 5),        # two discs
    ('d1', 45),             # two boxes, the SLEEP instantiation with allow_sleep=1
    ('d1_discs', 53),
    ('d2', 99),             # a GradientLight with its one-word light_action
    ('d2_discs', 89),
    ('d3', 121),            # SimplePhototaxis under a MomentumLight that a light_action pushes
    ('d3_discs', 125),      # ... under a CompositeLight (six words)
    ('d4', 145),
    ('d4_discs', 137),
    ('d5', 169),            # KB_DRIVE_MIXED
    ('d5w', 166),           # ... beyond 128 kilobots
])
FIXED = 'd0'
FORMS = ('fused', 'masked', 'set')      # step(10, actions);  step(1, env_mask, actions);  set_actions(actions) then step(3)
FORM_SUBSTEPS = {'fused': 10, 'masked': 1, 'set': 3}
STEP_OUTPUTS = ('x', 'y')               # what must move in every replay (SimplePhototaxis kilobots drive without turning)
MASKS = ([1, 0], [0, 1], [1, 1])        # the env_mask of replay k (E = 2)


def unit_of(variant):
    """The translation unit that holds an instantiation (the in_unit rules of csrc/kb_inst_*.hip)."""
    drive, light, obj, fn, tier, poly, sense, sleep = variant
    if drive == O.DRIVE_MIXED:
        return {1: 'd5', 3: 'd5w'}[tier]
    return 'd%d%s' % (drive, '' if poly else '_discs')


def units_in_tree():
    here = os.path.join(VC.ROOT, 'gym_kilobots_amd', 'csrc')
    return sorted(os.path.basename(p)[len('kb_inst_'):-len('.hip')] for p in glob.glob(os.path.join(here, 'kb_inst_*.hip')))


def step_row(unit):
    """The census row (inputs, index, variant) of a unit."""
    by_index = {row[1]: row for row in VC.rows()}
    return by_index[STEP_UNITS[unit]]


def takes_actions(s):
    return s.mode in (O.DRIVE_VELOCITY, O.DRIVE_ACCEL, O.DRIVE_MIXED)


def light_action_dim(s):
    return {O.LIGHT_NONE: 0, O.LIGHT_GRADIENT: 1, O.LIGHT_COMPOSITE: 6}.get(s.light, 2)


def step_inputs(s, k):
    """(actions [E, N, 2] or None, light_action [E, dim] or None, env_mask [E] uint8) of replay k of census scene s"""
    a = VC.stop_and_go_actions(s.E, s.N, k, seed=7) if takes_actions(s) else None
    dim = light_action_dim(s)
    la = np.random.RandomState(500 + k).uniform(-0.02, 0.02, (s.E, dim)).astype(np.float32) if dim else None
    return a, la, np.array(MASKS[k], np.uint8)


def oracle_form(osim, s, form, k):
    """Replay k of a form on the oracle."""
    from tests import reset_envs_ref as R
    a, la, mask = step_inputs(s, k)
    if a is not None:
        osim.set_actions(a)
    if form == 'masked':
        R.masked(osim, mask, lambda: osim.step(1, light_action=la))
    else:
        osim.step(FORM_SUBSTEPS[form], light_action=la)


# ---- resets ----------------------------------------------------------------------------------------------------------------
RESET_CASE = 'objects64'    # tests/reset_envs_ref.py: 4 envs of 64 Phototaxis kilobots, a disc, a box and a light
RESET_SEED = 2 ** 33 + 17
RESET_MASKS = ([1, 0, 1, 1], [0, 1, 1, 0], [1, 1, 0, 1])


def reset_inputs(k):
    """(env_mask [E] uint8, objects [E, M, 3], lights [E, 2]) of replay k of reset_envs: the templates of the case moved on"""
    from tests import reset_envs_ref as R
    objects, lights, _ = R.templates(RESET_CASE)
    shift = np.float32(0.25 * (k + 1))
    return np.array(RESET_MASKS[k], np.uint8), np.ascontiguousarray(objects + np.array([shift, -shift, 0.1 * (k + 1)], np.float32)), \
        np.ascontiguousarray(lights + np.float32(0.01 * (k + 1)))


# ---- the env ---------------------------------------------------------------------------------------------------------------
ENV_E, ENV_N, ENV_REPLAYS, ENV_EPISODE = 5, 64, 8, 3
ENV_GRID = (32, 24)
ENV_SLOTS = 12


def env_kw():
    """The keywords of the env row: every observation that runs on the device, a field, the two boxes, episodes of three steps."""
    rng = np.random.RandomState(41)
    points = (rng.uniform(-1.0, 1.0, (ENV_E, ENV_SLOTS, 2)) * [0.4, 0.3]).astype(np.float32)
    return dict(RS.BOXES, allow_sleep=0, spawn_std=0.12, seed=11, on_status='ignore', auto_reset=True, max_episode_steps=ENV_EPISODE,
                object_init=np.array([[0.1, 0.05, 0.2], [-0.15, -0.1, -0.3]]),
                neighbor_obs=(RS.RADIUS, 4), histogram_obs=(RS.RADIUS, 2, 4), comm_radius=RS.RADIUS, object_obs=True,
                grid_obs=ENV_GRID + (('count', 'flow', 'objects'),), coverage_obs=ENV_GRID, target_obs=(points, RS.TARGET_TOL),
                target_match=('greedy', 0.3), contact_obs=4, ray_obs=(0.2, 8), edge_obs=(RS.RADIUS, 2048), path_obs=ENV_GRID + (RS.CLEARANCE,),
                render_size=ENV_GRID, field_obs=ENV_GRID + (2,), field_keep=(0.95, 0.8), field_spread=(0.2, 0.1), field_iters=2)


ENV_GOAL = np.array([[0.8, 0.55]], np.float32)      # set_path_goal, before the capture
ENV_DONE_X = 0.1            # done_fn: the first kilobot of the env is further right than this, in metres
# the outputs of env.step that are floats of every kilobot's pose, by their place in (obs, reward, done, info): these must
# differ from one replay to the next.  (done, the counters and the integer outputs of the same launches take few values.)
ENV_MOVING = ('.0', '.1', '.3.terminal_obs', '.3.episode_return', '.3.neighbors.1', '.3.objects', '.3.walls', '.3.grid', '.3.coverage.dist',
              '.3.coverage.cells', '.3.targets.rel', '.3.targets.dist', '.3.targets.stats', '.3.paths.bots', '.3.rays.0', '.3.edges.rel',
              '.3.contacts.2', '.3.field')


def env_reward(prev, actions, obs):
    """reward_fn, done_fn and deposit_fn of the env row: torch only, on whatever device the poses live"""
    return (obs[..., :2] - prev[..., :2]).norm(dim=-1).sum(1)


def env_done(prev, actions, obs):
    return obs[:, 0, 0] > ENV_DONE_X


def env_deposit(prev, actions, obs):
    import torch
    return torch.stack((actions[..., 0] * 100.0, actions[..., 1].abs()), -1).contiguous()


def env_actions(k):
    return scenes.random_actions(ENV_E, ENV_N, seed=60 + k)


# ---- what cannot be captured -----------------------------------------------------------------------------------------------
# public method of KilobotSim -> why it is no row: it reads the device back, and raises ValueError inside a capture before any
# launch (the message names the way out)
REFUSED = {
    'host_state': 'one launch and a copy to the host: the point of the call',
    'status_bits': 'reads kb_buffers.status back',
    'check_status': "reads kb_buffers.status back unless mode='ignore', which launches nothing",
    'path_cells': 'bins the points on the host and uploads the mask',
}
# ... and the form of a row's method that is refused, while the row captures the other
REFUSED_FORMS = {'edges': 'capacity=None reads nnz back to size the lists'}
# ... and of BatchedKilobotsEnv
REFUSED_ENV = {
    '_check_status': "reads kb_buffers.status back unless on_status='ignore'",
    'set_targets': 'with points: checks them on the host and uploads them',
    'set_path_goal': 'takes the cells or the points through the host',
    'set_path_blocked': 'takes the cells through the host',
}
# public methods of KilobotSim that launch and are rows under another name, or that a row runs on the way
STEP_METHODS = {'step': 'STEP', 'set_actions': 'STEP', 'reset': 'RESETS', 'reset_envs': 'RESETS', 'poses': 'ENV'}
