"""BatchedKilobotsEnv: the tensor-level API for many envs on one GPU (what RL training loops use).

Same semantics as DirectControlKilobotsEnv / KilobotsEnv per env, but observations stay on the
device as torch tensors: poses [E, N, 3] (metres, radians), actions [E, N, 2]."""
import collections

import numpy as np
import torch

from .. import _native as nat
from ..lib.kilobot import Kilobot
from ..spaces import Box


def _neighbor_obs(value, num_objects):
    radius_m, k = value
    if not float(radius_m) > 0.0 or not 1 <= int(k) <= nat.MAX_NEIGHBORS:
        raise ValueError('neighbor_obs must be (radius_m > 0, 1 <= k <= %d)' % nat.MAX_NEIGHBORS)
    return float(radius_m), int(k)


def _histogram_obs(value, num_objects):
    radius_m, n_rings, n_sectors = value
    radius_m, grid = float(radius_m), nat.check_histogram_grid(n_rings, n_sectors)
    return (nat.check_radius(radius_m, 'histogram_obs: radius_m'),) + grid


def _object_obs(value, num_objects):
    if value not in (False, True):
        raise ValueError('object_obs must be True, False or None')
    return bool(value)


def _grid_obs(value, num_objects):
    width, height, planes = tuple(value) if len(value) == 3 else tuple(value) + (('count',),)
    grid = nat.check_grid(width, height, planes)
    if grid[2] & nat.GRID_OBJECTS and num_objects == 0:
        raise ValueError("grid_obs: 'objects' asked for, but the env has no objects")
    return grid


def _coverage_obs(value, num_objects):
    width, height = value
    return nat.check_coverage(width, height)


def _field_obs(value, num_objects):
    width, height, channels = tuple(value) if len(value) == 3 else tuple(value) + (1,)
    return nat.check_field(width, height, channels, 1.0, 0.0, 0)[:3]


def _target_obs(value, num_objects):
    points_m, tol_m = value
    points = np.ascontiguousarray(np.asarray(points_m.cpu() if torch.is_tensor(points_m) else points_m, dtype=np.float32))
    if points.ndim not in (2, 3) or points.shape[-1] != 2 or not np.isfinite(points).all():
        raise ValueError('target_obs: points_m must be finite and have the shape (K, 2) or (E, K, 2)')
    return (points,) + nat.check_targets(points.shape[-2], tol_m)[1:]


def _target_match(value):
    """target_match -- 'greedy' or ('greedy', cutoff_m) -- as the keywords KilobotSim.targets gets for it."""
    match, cutoff_m = (value, None) if isinstance(value, str) else tuple(value) if hasattr(value, '__len__') and len(value) == 2 else (None, None)
    if match != 'greedy':
        raise ValueError("target_match must be None, 'greedy' or ('greedy', cutoff_m)")
    cutoff_m = nat.check_assign(1, 0.0, cutoff_m)[2]
    return dict(match='greedy') if cutoff_m == float('inf') else dict(match='greedy', cutoff_m=cutoff_m)


def _path_obs(value, num_objects):
    width, height, clearance_m = tuple(value) if len(value) == 3 else tuple(value) + (0.0,)
    return nat.check_paths(width, height, clearance_m)


def _contact_obs(value, num_objects):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 0 <= value <= nat.MAX_CONTACT_SLOTS:
        raise ValueError('contact_obs must be an int in 0..%d or None' % nat.MAX_CONTACT_SLOTS)
    return int(value)


def _ray_obs(value, num_objects):
    radius_m, n_rays, targets = tuple(value) if len(value) == 3 else tuple(value) + (None,)
    if targets is None:
        targets = nat.RAY_BOTS | nat.RAY_WALLS | (nat.RAY_OBJECTS if num_objects > 0 else 0)
    rays = nat.check_rays(radius_m, n_rays, targets)
    if rays[2] & nat.RAY_OBJECTS and num_objects == 0:
        raise ValueError("ray_obs: 'objects' asked for, but the env has no objects")
    return rays


def _edge_obs(value, num_objects):
    return nat.check_edges(*(tuple(value) if hasattr(value, '__len__') else (value, None)))


def _render_size(value, num_objects):
    width, height = value
    return nat.check_render(width, height, nat.RENDER_BOTS)[:2]


# What an env can be created with besides the poses, a row per constructor keyword.  parse: the user's value (not None) to what
# the attribute of the keyword's name holds, a TypeError on the way becoming "<keyword> must be <shape>" where a shape is given.
# keys: where step() puts what the method of the sim returns for the stored value, in this order; none: step() leaves it to the
# accessor.  form, purpose: "create the env with <keyword>=<form> to <purpose>", for an accessor on an env created without it.
Option = collections.namedtuple('Option', ('parse', 'shape', 'keys', 'method', 'form', 'purpose'))
OPTIONS = {
    'neighbor_obs': Option(_neighbor_obs, None, ('neighbors',), 'neighbors', '(radius_m, k)', 'observe neighbours'),
    'histogram_obs': Option(_histogram_obs, '(radius_m, n_rings, n_sectors)', ('neighbor_histogram',), 'neighbor_histogram', '(radius_m, n_rings, n_sectors)', 'observe neighbour histograms'),
    'object_obs': Option(_object_obs, None, ('objects', 'walls'), 'object_points', 'True', 'observe objects and walls'),
    'grid_obs': Option(_grid_obs, '(width, height) or (width, height, planes)', ('grid',), 'occupancy_grid', '(width, height[, planes])', 'observe occupancy grids'),
    'coverage_obs': Option(_coverage_obs, '(width, height)', ('coverage',), 'coverage', '(width, height)', 'observe nearest-kilobot fields'),
    'field_obs': Option(_field_obs, '(width, height) or (width, height, channels)', (), None, '(width, height[, channels])', 'keep a pheromone field'),
    'target_obs': Option(_target_obs, '(points_m, tol_m)', ('targets',), 'targets', '(points_m, tol_m)', 'observe the slots of a target shape'),
    'path_obs': Option(_path_obs, '(width, height) or (width, height, clearance_m)', ('paths',), 'paths', '(width, height[, clearance_m])', 'observe distance-to-goal fields'),
    'contact_obs': Option(_contact_obs, None, ('contacts',), 'contacts', 'k', 'observe contacts'),
    'ray_obs': Option(_ray_obs, '(radius_m, n_rays) or (radius_m, n_rays, targets)', ('rays',), 'rays', '(radius_m, n_rays[, targets])', 'observe range scans'),
    'edge_obs': Option(_edge_obs, 'radius_m or (radius_m, capacity)', ('edges',), 'edges', 'radius_m or (radius_m, capacity)', 'observe the IR-range graph'),
    'render_size': Option(_render_size, '(width, height)', (), 'render', '(width, height)', 'render frames'),
    'comm_radius': Option(lambda value, num_objects: nat.check_radius(value, 'comm_radius'), 'a radius in metres', (), None, 'radius_m', None),
}


class BatchedKilobotsEnv(object):
    steps_per_action = 10            # kilobots_env.py:28
    sim_step = 0.1                   # kilobots_env.py:25,32

    def __init__(self, num_envs, num_kilobots, drive_mode=nat.DRIVE_VELOCITY, light_type=nat.LIGHT_NONE,
                 world_size=(2.0, 1.5), spawn_std=0.1, spawn_mean=(0.0, 0.0), seed=0, device=None,
                 sim_factory=None, reward_fn=None, env_offset=0, on_status='raise', status_interval=1, neighbor_obs=None, histogram_obs=None, comm_radius=None,
                 object_obs=None, grid_obs=None, coverage_obs=None, target_obs=None, contact_obs=None, render_size=None, ray_obs=None, edge_obs=None,
                 max_episode_steps=None, done_fn=None, auto_reset=False, object_init=None, light_init=None,
                 field_obs=None, field_keep=1.0, field_spread=0.0, field_iters=1, deposit_fn=None, path_obs=None, target_match=None, **cfg):
        """env_offset: global index of this shard's first env (multi-GPU: the Philox counters of reset() are keyed by the
        GLOBAL env index, so a shard equals the corresponding rows of the unsharded batch).
        on_status / status_interval: capacity overflows of the device step (kb_buffers.status) are checked after
        reset() and after every status_interval-th step(): 'raise' | 'warn' | 'ignore' (one 4-byte device read each).
        neighbor_obs: (radius_m, k) adds the IR-range observation of a decentralised policy: neighbors() returns the k
        nearest kilobots within radius_m of every kilobot in its own frame (KilobotSim.neighbors), and step() puts them
        in its info dict under 'neighbors'.  None: reset() and step() are what they were, the info dict stays {}.
        histogram_obs: (radius_m, n_rings, n_sectors) adds the fixed-size local histogram of ALL kilobots in range, binned by
        distance and bearing in the kilobot's own frame (KilobotSim.neighbor_histogram): neighbor_histogram() returns it,
        step() puts it in its info dict under 'neighbor_histogram'.  Independent of neighbor_obs; None adds nothing.
        comm_radius: the IR range in metres over which neighbor_reduce(values) aggregates what the kilobots broadcast
        (KilobotSim.neighbor_reduce) and over which hops(seeds) forms hop-count gradients (KilobotSim.hops) and clusters() labels the
        connected components (KilobotSim.clusters).  reset() and step() do not change with it.
        object_obs: True adds what a kilobot sees of the objects and the walls: object_points() returns the nearest point of
        every object and of the arena walls in every kilobot's own frame (KilobotSim.object_points), and step() puts them in
        its info dict under 'objects' (envs with objects only) and 'walls'.  None (or False): nothing is added.
        grid_obs: (width, height) or (width, height, planes) adds what a CENTRAL policy is fed, a fixed-size image of the
        whole table: occupancy_grid() returns [E, C, height, width] (KilobotSim.occupancy_grid; planes made of 'count',
        'flow' and 'objects', default ('count',)), and step() puts it in its info dict under 'grid'.  None adds nothing.
        coverage_obs: (width, height) adds the nearest-kilobot fields of a coverage or dispersion task: coverage() returns the
        named tuple (owner [E, height, width], dist [E, height, width], cells [E, N, 4], stats [E, 2]) of KilobotSim.coverage --
        which kilobot is nearest to every cell centre of the table and how far, the Voronoi cell of every kilobot with its
        centroid in the kilobot's own frame, the locational cost and the worst-covered distance -- and step() puts the tuple in
        its info dict under 'coverage'.  None adds nothing.
        target_obs: (points_m, tol_m) adds the observation of a shape-formation task, the matching between the kilobots and the K
        points ("slots") of a target shape: points_m array-like [K, 2] (one shape for all envs) or [E, K, 2], metres, uploaded
        once; targets() returns the named tuple (index [E, N], rel [E, N, 4], owner [E, K], dist [E, K], stats [E, 6]) of
        KilobotSim.targets -- the nearest slot of every kilobot in its own frame and whether it holds it, the nearest kilobot
        of every slot and how far it is, the Chamfer sums, Hausdorff distances and the counts within tol_m the reward is made
        of -- and step() puts the tuple in its info dict under 'targets'.  set_targets() replaces the points or masks slots
        out.  None adds nothing.
        target_match: 'greedy' or ('greedy', cutoff_m) makes targets() and info['targets'] the ONE-TO-ONE greedy matching of
        kilobots and slots instead (KilobotSim.targets with match='greedy': index the slot matched to a kilobot or -1, owner the
        kilobot matched to a slot or -1, stats the sums over the matched pairs, no pair further apart than cutoff_m).  Needs
        target_obs.  None: the nearest queries, as before.
        contact_obs: k, an int in 0..16, adds touch and push sensing from the contacts the solver acted on in the last world
        step: contacts() returns (partner [E, N, k], impulse [E, N, k], touch [E, N, 4], obj [E, M, 2] or None)
        (KilobotSim.contacts; k = 0: no lists, partner and impulse are None), and step() puts the tuple in its info dict under
        'contacts'.  None adds nothing.
        render_size: (width, height) in pixels lets render('rgb_array') return the frames of every env, [E, height, width, 3]
        uint8 on the device (KilobotSim.render).  reset(), step() and the info dict do not change with it.
        path_obs: (width, height) or (width, height, clearance_m) adds the obstacle-aware distance-to-goal field of a pushing or
        navigation task: paths() returns the named tuple (dist [E, height, width], step [E, height, width], bots [E, N, 4],
        stats [E, 4]) of KilobotSim.paths -- the shortest-path distance of every cell to the goal round the objects, the
        direction of descent, and for every kilobot the metres still to go and the way in its own frame -- and step() puts
        the tuple in its info dict under 'paths'.  set_path_goal() sets the goal (positions or cells), set_path_blocked()
        further blocked cells; without a goal every kilobot is unreachable.
        ray_obs: (radius_m, n_rays) or (radius_m, n_rays, targets) adds the range scan of a decentralised policy: rays() returns
        (dist [E, N, n_rays], hit [E, N, n_rays]), how far the first kilobot, object or wall along each of n_rays bearings in
        every kilobot's own frame is and what it is (KilobotSim.rays; targets made of 'bots', 'objects' and 'walls', default:
        everything the env has), and step() puts the tuple in its info dict under 'rays'.  None adds nothing.
        edge_obs: radius_m or (radius_m, capacity) adds the whole IR-range graph, for graph-network policies: edges() returns
        the named tuple (src, dst, rel, offsets, count, nnz) of KilobotSim.edges -- every pair of kilobots in range as a
        CSR / COO edge list over the batch, node e * N + i for kilobot i of env e; with a capacity the lists have that fixed
        length and nothing is read back from the device, without one they have nnz entries at the price of one read -- and
        step() puts the tuple in its info dict under 'edges'.  None adds nothing.
        field_obs: (width, height) or (width, height, channels) gives every env a pheromone field, the memory of a stigmergy
        task (trails, foraging, area marking): env.field [E, channels, height, width] lies over the arena like the grid of
        grid_obs.  After the world step, step() lets every kilobot deposit into the cell it stands in, diffuses and decays the
        field field_iters times with field_keep and field_spread (a number or one per channel) and puts what every kilobot
        reads, [E, N, channels, 4] = (value, gradient per metre ahead, to the left, what its cell just received), in its info
        dict under 'field' -- all in one launch (KilobotSim.field_step).  deposit_fn(prev_obs, actions, obs) returns the amounts
        [E, N] or [E, N, channels]; None: every kilobot deposits 1.0 in every channel.  reset() zeroes the field, reset_envs()
        that of the envs it selects; with auto_reset the rows of an env that was just reset are read off its zeroed planes.
        field_sense() reads the rows without changing the field.  None adds nothing.
        Episodes of single envs, all off by default (reset(), step() and the info dict are then what they were):
        max_episode_steps: an env is done once it has taken that many steps since its last reset.
        done_fn: called as done_fn(prev, actions, obs) like reward_fn, returns a bool tensor [E]: the envs that are done.
        With either, step() reports done = done_fn(...) | (episode_steps >= max_episode_steps) and puts 'episode_return' and
        'episode_length' ([E], final for the done envs) in its info dict.
        auto_reset: step() resets the done envs (reset_envs) before it takes the observations: obs and every observation in
        the info dict describe the new episode, info['terminal_obs'] holds the poses from before the reset.
        object_init: [E, M, 3] or [M, 3] (x [m], y [m], theta): where reset() and reset_envs() put the objects, at rest;
        converted once, as KilobotSim.set_objects_m converts.  None: resets leave the objects alone.
        light_init: [E, L, 2], [L, 2] or [2] metres (a GradientLight: its angle first): where they put the lights, with
        velocity 0.  None: resets leave the lights alone.
        Nothing on this path reads the device back: a step in which no env is done costs two small launches."""
        if sim_factory is None:
            from ..sim import KilobotSim as sim_factory
        if on_status not in ('raise', 'warn', 'ignore'):
            raise ValueError("on_status must be 'raise', 'warn' or 'ignore'")
        self.num_envs, self.num_kilobots = int(num_envs), int(num_kilobots)
        self.world_width, self.world_height = world_size
        self.spawn_std, self.spawn_mean = spawn_std, np.asarray(spawn_mean, dtype=np.float64)
        if seed is None:        # (gym convention: no seed given -> draw one; the device reset needs an integer key)
            seed = int(np.random.SeedSequence().entropy) & 0x7FFFFFFF
        self._rng = np.random.RandomState(seed)
        self._seed = seed
        self._resets = 0
        self.env_offset = int(env_offset)
        self._on_status, self._status_interval, self._steps = on_status, max(1, int(status_interval)), 0
        self.reward_fn = reward_fn
        given = dict(neighbor_obs=neighbor_obs, histogram_obs=histogram_obs, comm_radius=comm_radius, object_obs=object_obs, grid_obs=grid_obs, coverage_obs=coverage_obs, target_obs=target_obs,
                     contact_obs=contact_obs, render_size=render_size, ray_obs=ray_obs, edge_obs=edge_obs, field_obs=field_obs, path_obs=path_obs)
        for name, option in OPTIONS.items():
            value = given[name]
            if value is not None:
                try:
                    value = option.parse(value, int(cfg.get('num_objects', 0)))
                except TypeError as err:
                    if option.shape is None:
                        raise
                    raise ValueError('%s must be %s: %s' % (name, option.shape, err))
            setattr(self, name, value)
        self.object_obs = bool(self.object_obs)         # (the one keyword that is off as False)
        self._target_kw = {} if target_match is None else _target_match(target_match)       # what targets() gets besides the slot mask
        if target_match is not None and self.target_obs is None:
            raise ValueError('target_match needs target_obs=(points_m, tol_m)')
        kw = dict(cfg)
        if 'contact_capacity' not in kw:
            # a Gaussian cloud of std s overlaps N (N - 1) / 2 * (1 - exp(-r^2 / s^2)) pairs at spawn: size the contact
            # store for it (entries live in HBM), so that the reference's default spawn never drops contacts silently
            r, n = float(kw.get('bot_radius', 0.0165)), self.num_kilobots
            pairs = 0.5 * n * (n - 1) * (1.0 - np.exp(-(r * r) / max(float(spawn_std) ** 2, 1e-12)))
            default_cap = max(4 * n + 64, min(n * (n - 1) // 2 + 4 * n, 2304))
            need = int(1.5 * pairs) + 4 * n + 64
            if need > default_cap:
                kw['contact_capacity'] = min(need, n * (n - 1) // 2 + 4 * n, 65528)
                kw.setdefault('ws_slots', 64)
        if device is not None:
            kw['device'] = device
        self.sim = sim_factory(self.num_envs, self.num_kilobots, drive_mode, light_type,
                               world_width=self.world_width, world_height=self.world_height, **kw)
        lo = np.array([0.0, -Kilobot._max_angular_velocity])
        hi = np.array([Kilobot._max_linear_velocity, Kilobot._max_angular_velocity])
        if drive_mode == nat.DRIVE_ACCEL:
            lo, hi = np.array([-.005, -.2 * np.pi]), np.array([.005, .2 * np.pi])
        self.action_space = Box(np.tile(lo, (self.num_kilobots, 1)), np.tile(hi, (self.num_kilobots, 1)), dtype=np.float64)
        b = np.array([self.world_width / 2, self.world_height / 2, np.inf])
        self.observation_space = Box(np.tile(-b, (self.num_kilobots, 1)), np.tile(b, (self.num_kilobots, 1)), dtype=np.float32)
        dev = self.sim.x.device
        self.episode_returns = torch.zeros(self.num_envs, dtype=torch.float32, device=dev)
        self._observe_kw = {}       # keyword arguments the sim method of an observation gets besides the stored value
        if self.target_obs is not None:         # the points live on the device from here on: (tensor, tol_m)
            self.target_obs = (self._target_points(self.target_obs[0]), self.target_obs[1])
            if self._target_kw:
                self._observe_kw['target_obs'] = dict(self._target_kw)
        if self.path_obs is not None:           # (width, height) from here on; the goal and the blocked cells live on the device
            width, height, clearance_m = self.path_obs
            self.path_obs = (width, height)
            self._observe_kw['path_obs'] = dict(source=torch.zeros(self.num_envs, height, width, dtype=torch.uint8, device=dev), blocked=None,
                                                clearance_m=clearance_m)
        self.field, self.deposit_fn = None, deposit_fn
        if self.field_obs is not None:          # the env owns the field; keep, spread and iters are checked once, here
            self._field_kw = dict(zip(('keep', 'spread', 'iters'), nat.check_field(*self.field_obs, field_keep, field_spread, field_iters)[3:]))
            self.field = self.sim.new_field(*self.field_obs)
            self._field_ones = torch.ones(self.num_envs, self.num_kilobots, self.field_obs[2], dtype=torch.float32, device=dev)
        # episodes of single envs
        if max_episode_steps is not None and not int(max_episode_steps) >= 1:
            raise ValueError('max_episode_steps must be at least 1 or None')
        self.max_episode_steps = None if max_episode_steps is None else int(max_episode_steps)
        self.done_fn, self.auto_reset = done_fn, bool(auto_reset)
        self._episodes = self.max_episode_steps is not None or done_fn is not None or self.auto_reset
        self.episode_steps = torch.zeros(self.num_envs, dtype=torch.int32, device=dev)
        self.episode_index = torch.zeros(self.num_envs, dtype=torch.int32, device=dev)    # word z of the spawn's Philox counter
        self._reset_key = None
        self._object_init = self._light_init = None
        E, M = self.num_envs, int(cfg.get('num_objects', 0))
        if object_init is not None:
            a = np.asarray(object_init.cpu() if torch.is_tensor(object_init) else object_init, np.float64)
            if M == 0 or a.shape not in ((E, M, 3), (M, 3)):
                raise ValueError('object_init must have the shape %s or %s in an env with objects' % ((E, M, 3), (M, 3)))
            a = np.broadcast_to(a, (E, M, 3))
            w = np.empty((E, M, 3), np.float32)
            w[..., :2] = (a[..., :2] * nat.WORLD_SCALE).astype(np.float32)      # (as set_objects_m: float64 metres x 25, then rounded)
            w[..., 2] = a[..., 2].astype(np.float32)
            self._object_init = torch.from_numpy(w).to(dev)
        if light_init is not None:
            if self.sim.light_x is None or light_type == nat.LIGHT_NONE:
                raise ValueError('light_init given, but the env has no light')
            shape = tuple(self.sim.light_x.shape) + (2,)
            a = np.asarray(light_init.cpu() if torch.is_tensor(light_init) else light_init, np.float32)
            if a.shape not in (shape, shape[1:], (2,)):
                raise ValueError('light_init must have the shape %s, %s or (2,)' % (shape, shape[1:]))
            self._light_init = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, shape))).to(dev)

    def seed(self, seed=None):
        if seed is not None:
            self._seed = seed
            self._rng = np.random.RandomState(seed)
            self._resets = 0
        return [self._seed]

    def _check_status(self, where):
        if self._on_status == 'ignore':
            return
        nat.refuse_capture('%s with on_status=%r' % (where, self._on_status), "create the env with on_status='ignore' and check sim.status outside the capture")
        bits = self.sim.status_bits()
        if not bits:
            return
        nat.report_status(self._on_status, where, bits)
        self.sim.status.zero_()

    def spawn(self):
        """YamlKilobotsEnv._init_kilobots spawn rule (yaml_kilobots_env.py:346-352), theta = 0 (body.py:28-29)."""
        E, N = self.num_envs, self.num_kilobots
        xy = self._rng.normal(scale=self.spawn_std, size=(E, N, 2)) + self.spawn_mean
        lo = np.array([-self.world_width / 2, -self.world_height / 2]) + 0.02
        hi = np.array([self.world_width / 2, self.world_height / 2]) - 0.02
        return np.minimum(np.maximum(xy, lo), hi), np.zeros((E, N))

    def reset(self, poses=None):
        """poses: optional (xy [E,N,2] metres, theta [E,N]) uploaded from the host.  Default: the reference's Gaussian
        spawn drawn ON THE DEVICE (kb_reset: Philox4x32-10 keyed by (seed + reset count; global env, bot)), no host
        arrays, no H2D copy; followed by the "step to resolve" of kilobots_env.py:156-157 either way."""
        templates = self._object_init is not None or self._light_init is not None
        self._reset_key = (int(self._seed) << 20) + self._resets       # (reset_envs draws the later episodes from the same key)
        if poses is None:
            kw = dict(seed=self._reset_key, mean=tuple(float(v) for v in self.spawn_mean),
                      std=float(self.spawn_std), random_theta=False, random_velocity=False, resolve=True,
                      env_offset=self.env_offset)
            if templates:       # the spawn of sim.reset() (counter word 0) with the objects and lights put in place before the resolve step
                self.sim.reset_envs(torch.ones(self.num_envs, dtype=torch.bool, device=self.episode_index.device),
                                    objects=self._object_init, lights=self._light_init, **kw)
            else:
                self.sim.reset(**kw)
            self._resets += 1
        else:
            xy, th = poses
            self.sim.set_poses_m(xy, th)
            if templates:
                self._place_templates()
            self.sim.status.zero_()
            self.sim.step(1, flags=nat.STEP_NO_DRIVE)       # "step to resolve", kilobots_env.py:156-157
        self.episode_returns.zero_()
        self.episode_steps.zero_()
        self.episode_index.zero_()
        if self.field is not None:
            self.field.zero_()
        self._steps = 0
        self._check_status('reset()')
        return self.sim.poses()

    def _place_templates(self):
        """object_init / light_init into every env, at rest: what reset_envs does for the envs it selects."""
        s = self.sim
        if self._object_init is not None:
            s.ox.copy_(self._object_init[..., 0])
            s.oy.copy_(self._object_init[..., 1])
            s.otheta.copy_(self._object_init[..., 2])
            for t in (s.ovx, s.ovy, s.ow, s.osleep):
                if t is not None:
                    t.zero_()
            s.forget_contacts()
        if self._light_init is not None:
            s.light_x.copy_(self._light_init[..., 0])
            if s.light_y is not None:
                s.light_y.copy_(self._light_init[..., 1])
            for t in (s.light_vx, s.light_vy):
                if t is not None:
                    t.zero_()

    def reset_envs(self, env_mask):
        """Start a new episode in the envs env_mask selects ([E] bool or uint8 tensor on the sim's device); the others run on
        untouched (KilobotSim.reset_envs).  The spawn comes from the key of the last reset() and the counter word
        episode_index[e], which reset() zeroes and this call increments for the selected envs first: the j-th episode of
        global env e is a pure function of (seed, reset count, e, j), whenever the other envs end, sharded or not.  Puts the
        objects and lights at object_init / light_init, takes the step to resolve in those envs alone, zeroes their
        episode_returns and episode_steps, and returns the poses [E, N, 3] of all envs.  Nothing is read back from the device."""
        if self._reset_key is None:
            raise ValueError('reset_envs: call reset() first')
        sel = env_mask if env_mask.dtype == torch.bool else env_mask.ne(0)
        self.episode_index += sel.to(torch.int32)
        self.sim.reset_envs(env_mask, seed=self._reset_key, mean=tuple(float(v) for v in self.spawn_mean), std=float(self.spawn_std),
                            random_theta=False, random_velocity=False, resolve=True, env_offset=self.env_offset,
                            episode=self.episode_index, objects=self._object_init, lights=self._light_init)
        self.episode_returns.masked_fill_(sel, 0.0)
        self.episode_steps.masked_fill_(sel, 0)
        if self.field is not None:
            self.field.masked_fill_(sel.view(-1, 1, 1, 1), 0.0)
        return self.sim.poses()

    def step(self, actions=None, light_action=None):
        """actions [E, N, 2] float32 tensor on the sim's device (None keeps the previous commands).
        With on_status='ignore' the whole call can be captured into a graph (torch.cuda.graph) and replayed: INTEGRATION.md,
        "Capturing a step in a graph"."""
        if self._on_status != 'ignore':         # (the count of steps that decides when the status is read stops at capture: refused before any launch)
            nat.refuse_capture('step() with on_status=%r' % self._on_status, "create the env with on_status='ignore' and check sim.status outside the capture")
        prev =self.sim.poses() if self.reward_fn is not None or self.done_fn is not None or self.deposit_fn is not None else None
        self.sim.step(self.steps_per_action, actions=actions, light_action=light_action)
        obs = self.sim.poses()
        if self.reward_fn is not None:
            reward = self.reward_fn(prev, actions, obs)
        else:
            reward = torch.zeros(self.num_envs, dtype=torch.float32, device=obs.device)
        self.episode_returns += reward
        self._steps += 1
        if self._steps % self._status_interval == 0:
            self._check_status('step()')
        done = torch.zeros(self.num_envs, dtype=torch.bool, device=obs.device)
        info = {}
        if self._episodes:
            self.episode_steps += 1
            if self.done_fn is not None:
                done = done | self.done_fn(prev, actions, obs)
            if self.max_episode_steps is not None:
                done = done | (self.episode_steps >= self.max_episode_steps)
            info['episode_return'], info['episode_length'] = self.episode_returns.clone(), self.episode_steps.clone()
            if self.auto_reset:     # before the observations are taken: they describe the new episode
                info['terminal_obs'] = obs
                obs = self.reset_envs(done)
        for name, option in OPTIONS.items():
            value = getattr(self, name)
            if option.keys and value is not None and value is not False:      # (by identity: contact_obs=0 is an observation)
                out = self._observe(name)
                if len(option.keys) > 1 and not torch.is_tensor(out):
                    info.update(zip(option.keys, out))
                else:       # (object_points of an env without objects returns the walls alone)
                    info[option.keys[-1]] = out
        if self.field is not None:
            amount = self._field_ones if self.deposit_fn is None else self.deposit_fn(prev, actions, obs)
            if self._episodes and self.auto_reset:
                # the envs that run on take the update; those that were just reset start from their zeroed planes, and their
                # rows are read off them: two launches into one tensor, the masks stay on the device
                rows = self.sim.field_step(self.field, amount, env_mask=~done, **self._field_kw)
                info['field'] = self.sim.field_step(self.field, None, iters=0, env_mask=done, out=rows)
            else:
                info['field'] = self.sim.field_step(self.field, amount, **self._field_kw)
        return obs, reward, done, info

    def _stored(self, name, purpose=None):
        """What the env holds for the constructor keyword `name`; ValueError if it was created without it."""
        value = getattr(self, name)
        if value is None or value is False:
            raise ValueError('create the env with %s=%s to %s' % (name, OPTIONS[name].form, purpose or OPTIONS[name].purpose))
        return value

    def _observe(self, name):
        value = self._stored(name)      # the tuple of the sim method's arguments, its one argument, or True for none
        args = value if isinstance(value, tuple) else (value,) if value is not True else ()
        return getattr(self.sim, OPTIONS[name].method)(*args, **self._observe_kw.get(name, {}))

    def neighbors(self):
        """(index [E, N, k] int32, rel [E, N, k, 4] float32, count [E, N] int32) of the current poses for the
        neighbor_obs=(radius_m, k) the env was created with: KilobotSim.neighbors."""
        return self._observe('neighbor_obs')

    def neighbor_histogram(self):
        """hist [E, N, n_rings, n_sectors] float32 of the current poses for the histogram_obs=(radius_m, n_rings, n_sectors)
        the env was created with: KilobotSim.neighbor_histogram."""
        return self._observe('histogram_obs')

    def object_points(self):
        """(obj [E, N, M, 4], wall [E, N, 4]) float32 of the current poses -- wall alone in an env without objects -- for
        an env created with object_obs=True: KilobotSim.object_points."""
        return self._observe('object_obs')

    def occupancy_grid(self):
        """grid [E, C, height, width] float32 of the current poses for the grid_obs=(width, height[, planes]) the env was
        created with: KilobotSim.occupancy_grid."""
        return self._observe('grid_obs')

    def coverage(self):
        """The named tuple (owner [E, height, width] int32, dist [E, height, width] float32, cells [E, N, 4] float32, stats
        [E, 2] float32) of the current poses for the coverage_obs=(width, height) the env was created with:
        KilobotSim.coverage."""
        return self._observe('coverage_obs')

    def field_sense(self):
        """sense [E, N, channels, 4] float32 of the current poses on env.field as it is, for the field_obs=(width, height[,
        channels]) the env was created with: KilobotSim.field_step as a pure read (nothing is deposited, the field does not
        change, the fourth word is 0)."""
        self._stored('field_obs')
        return self.sim.field_step(self.field, None, iters=0)

    def _target_points(self, points):
        """Parsed points ([K, 2] or [E, K, 2] float32 array) on the sim's device; ValueError if they do not fit the env."""
        if points.ndim == 3 and points.shape[0] != self.num_envs:
            raise ValueError('target_obs: points_m must have the shape (K, 2) or (%d, K, 2)' % self.num_envs)
        return torch.from_numpy(points).to(self.sim.x.device)

    def set_targets(self, points_m=None, slot_select=None):
        """Replace the points of target_obs -- array-like [K, 2] or [E, K, 2] metres with the K the env was created with; None
        keeps them -- and set the slots that take part: slot_select [E, K] bool or uint8 tensor on the sim's device, None:
        all of them (KilobotSim.targets).  A reward that masks out the slots that are filled sets the mask here."""
        points, tol_m = self._stored('target_obs')
        if points_m is not None:
            nat.refuse_capture('set_targets(points_m)', 'it checks the points on the host and uploads them; call it before the capture and write into env.target_obs[0] in place')
            new = _target_obs((points_m, tol_m), 0)[0]
            if new.shape[-2] != points.shape[-2]:
                raise ValueError('set_targets: the env was created with %d slots, got %d' % (points.shape[-2], new.shape[-2]))
            self.target_obs = (self._target_points(new), tol_m)
        self._observe_kw['target_obs'] = dict(self._target_kw) if slot_select is None else dict(self._target_kw, slot_select=slot_select)

    def targets(self):
        """The named tuple (index [E, N] int32, rel [E, N, 4] float32, owner [E, K] int32, dist [E, K] float32, stats [E, 6]
        float32) of the current poses for the target_obs=(points_m, tol_m) the env was created with, over the slots
        set_targets() selected: KilobotSim.targets, the nearest queries or with target_match the greedy matching."""
        return self._observe('target_obs')

    def _path_mask(self, cells, name):
        """A caller's cell mask, array-like or tensor [height, width] or [E, height, width], as uint8 [E, height, width] on the
        sim's device."""
        width, height = self._stored('path_obs')
        nat.refuse_capture(name + '()', 'it takes the cells through the host; call it before the capture and write into the mask in place')
        t = torch.as_tensor(cells.cpu().numpy() if torch.is_tensor(cells) else np.asarray(cells))
        if t.dim() not in (2, 3) or tuple(t.shape[-2:]) != (height, width) or (t.dim() == 3 and t.shape[0] != self.num_envs):
            raise ValueError('%s: cells must have the shape (%d, %d) or (%d, %d, %d)' % (name, height, width, self.num_envs, height, width))
        return t.ne(0).to(torch.uint8).expand(self.num_envs, height, width).contiguous().to(self.sim.x.device)

    def set_path_goal(self, points_m=None, cells=None):
        """Set the goal of path_obs: points_m array-like [K, 2] or [E, K, 2] metres, the cells they fall in
        (KilobotSim.path_cells), or cells, a mask [height, width] or [E, height, width] of the goal cells; exactly one of
        the two.  An env is created without a goal: every kilobot is unreachable until one is set."""
        width, height = self._stored('path_obs')
        nat.refuse_capture('set_path_goal()', 'it takes the goal through the host; call it before the capture and write into the mask in place')
        if (points_m is None) == (cells is None):
            raise ValueError('set_path_goal: give either points_m or cells')
        self._observe_kw['path_obs']['source'] = self.sim.path_cells(points_m, width, height) if cells is None else self._path_mask(cells, 'set_path_goal')

    def set_path_blocked(self, cells):
        """Set the cells that block the paths of path_obs besides the objects: a mask [height, width] or [E, height, width];
        None: none."""
        self._stored('path_obs')
        self._observe_kw['path_obs']['blocked'] = None if cells is None else self._path_mask(cells, 'set_path_blocked')

    def paths(self):
        """The named tuple (dist [E, height, width] float32, step [E, height, width] int8, bots [E, N, 4] float32, stats [E, 4]
        float32) of the current poses for the path_obs=(width, height[, clearance_m]) the env was created with, to the goal
        of set_path_goal() round the objects and the cells of set_path_blocked(): KilobotSim.paths."""
        return self._observe('path_obs')

    def contacts(self):
        """(partner [E, N, k] int32, impulse [E, N, k] float32, touch [E, N, 4] float32, obj [E, M, 2] float32 or None) of the
        contacts of the last world step for the contact_obs=k the env was created with: KilobotSim.contacts."""
        return self._observe('contact_obs')

    def rays(self):
        """(dist [E, N, n_rays] float32, hit [E, N, n_rays] int32) of the current poses for the ray_obs=(radius_m, n_rays[,
        targets]) the env was created with: KilobotSim.rays."""
        return self._observe('ray_obs')

    def edges(self):
        """The named tuple (src, dst, rel, offsets, count, nnz) of the current poses for the edge_obs=radius_m or
        (radius_m, capacity) the env was created with: KilobotSim.edges."""
        return self._observe('edge_obs')

    def render(self, mode='rgb_array'):
        """frames [E, height, width, 3] uint8 of the current state for the render_size=(width, height) the env was created
        with: KilobotSim.render.  Only mode 'rgb_array' exists: there is no window."""
        if mode != 'rgb_array':
            raise NotImplementedError("BatchedKilobotsEnv.render: only mode 'rgb_array' (got %r)" % (mode,))
        return self._observe('render_size')

    def neighbor_reduce(self, values, op='sum', scale=65536.0, count=False):
        """What every kilobot hears of `values` ([E, N] or [E, N, C] float32 on the device) over the comm_radius the env
        was created with, combined by op ('sum' | 'min' | 'max'): KilobotSim.neighbor_reduce."""
        radius_m = self._stored('comm_radius', 'aggregate messages')
        return self.sim.neighbor_reduce(values, radius_m, op=op, scale=scale, count=count)

    def hops(self, seeds, max_hops=None, parent=False, root=False, stats=False):
        """The hop-count gradient of every kilobot to the nearest of `seeds` ([E, N] bool or uint8 on the device) over the
        comm_radius the env was created with: KilobotSim.hops."""
        radius_m = self._stored('comm_radius', 'form hop-count gradients')
        return self.sim.hops(seeds, radius_m, max_hops=max_hops, parent=parent, root=root, stats=stats)

    def clusters(self, select=None, size=False, table=False, stats=False):
        """The connected components of the kilobots (those of `select`, [E, N] bool or uint8 on the device; None: all) over the
        comm_radius the env was created with: KilobotSim.clusters."""
        radius_m = self._stored('comm_radius', 'label connected components')
        return self.sim.clusters(radius_m, select=select, size=size, table=table, stats=stats)

    def gather_episode_returns(self, dist=None):
        """Per-env returns of every rank's shard in global env order (the only collective)."""
        from ..dist import gather_returns
        return gather_returns(self.episode_returns, dist)

    def close(self):
        self.sim.close()
