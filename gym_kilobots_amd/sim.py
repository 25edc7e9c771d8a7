"""KilobotSim: device buffers (torch-ROCm tensors) + the HIP world step behind the C ABI.

This is the host side of the hot path only.  torch is used for device memory and streams; all
simulation arithmetic happens inside libkilobots_hip.so (gym_kilobots_amd/csrc/).
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _native as nat
from ._native import STATUS_BITS, KilobotsStatusError, describe_status  # noqa: F401
from ._native import (DRIVE_VELOCITY, DRIVE_ACCEL, DRIVE_MOTORS, DRIVE_SIMPLE_PHOTOTAXIS,  # noqa: F401
                      DRIVE_PHOTOTAXIS, LIGHT_NONE, LIGHT_CIRCULAR, STEP_NO_DRIVE, WORLD_SCALE)

# what KilobotSim.edges returns
Edges = collections.namedtuple('Edges', ('src', 'dst', 'rel', 'offsets', 'count', 'nnz'))
# ... and KilobotSim.coverage
Coverage = collections.namedtuple('Coverage', ('owner', 'dist', 'cells', 'stats'))
# ... and KilobotSim.targets
Targets = collections.namedtuple('Targets', ('index', 'rel', 'owner', 'dist', 'stats'))
# ... and KilobotSim.paths
Paths = collections.namedtuple('Paths', ('dist', 'step', 'bots', 'stats'))

# the dtypes a caller's tensor may have: floats, a mask (env_mask, seeds) and 32-bit words (colours, episode counters)
F32, I32, I64, MASK = (torch.float32,), (torch.int32,), (torch.int64,), (torch.bool, torch.uint8)
WORD = (torch.int32, getattr(torch, 'uint32', torch.int32))


def _ptr(t):
    """The device pointer of a tensor as the integer ctypes takes for a void *, None (NULL) for an absent one."""
    return None if t is None else t.data_ptr()


def _reset_params(seed, mean, std, random_theta, random_velocity, resolve, env_offset):
    rp = nat.KbResetParams()
    rp.seed, rp.env_offset = int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_offset)
    rp.mean[0], rp.mean[1], rp.std = float(mean[0]), float(mean[1]), float(std)
    rp.random_theta, rp.random_velocity, rp.resolve = int(bool(random_theta)), int(bool(random_velocity)), int(bool(resolve))
    return rp


class KilobotSim:
    """num_envs independent worlds of num_bots kilobots, resident on one GPU.

    State tensors are [num_envs, num_bots] float32 in Box2D world units (metres x 25), exactly
    what the reference's b2Body objects hold; `poses()` returns metres like Body.get_pose
    (reference gym_kilobots/lib/body.py:63-65).
    """

    def __init__(self, num_envs, num_bots, drive_mode=DRIVE_VELOCITY, light_type=LIGHT_NONE,
                 device=None, debug_outputs=False, **cfg_overrides):
        self._lib = nat.load()                      # raises if the HIP library is not built
        if not torch.cuda.is_available():
            raise nat.KilobotsHipError('KilobotSim needs a ROCm GPU (torch.cuda.is_available() is False); '
                                       'there is no CPU fallback')
        self.device = torch.device(device if device is not None else 'cuda:%d' % torch.cuda.current_device())
        if self.device.index is None:
            self.device = torch.device('cuda:%d' % torch.cuda.current_device())
        self.cfg = nat.default_config(num_envs, num_bots, drive_mode, light_type, **cfg_overrides)
        self.num_envs, self.num_bots = num_envs, num_bots
        self.drive_mode, self.light_type = drive_mode, light_type
        self._h = C.c_void_p()
        nat.call(self._lib, 'kb_create', C.byref(self.cfg), C.byref(self._h))
        E, N = num_envs, num_bots
        dev = self.device
        f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.x, self.y, self.theta = f(E, N), f(E, N), f(E, N)
        self.v = self.w = self.acc_v = self.acc_w = None
        self.motor_l = self.motor_r = None
        self.pt_threshold = self.pt_update = self.pt_nochange = self.pt_dir = None
        self.light_x = self.light_y = None
        mixed = drive_mode == nat.DRIVE_MIXED      # every per-law state buffer + the per-kilobot law
        self.bot_mode = torch.full((E, N), DRIVE_MOTORS, dtype=torch.uint8, device=dev) if mixed else None
        if drive_mode in (DRIVE_VELOCITY, DRIVE_ACCEL) or mixed:
            self.v, self.w = f(E, N), f(E, N)
        if drive_mode == DRIVE_ACCEL or mixed:
            self.acc_v, self.acc_w = f(E, N), f(E, N)
        if drive_mode in (DRIVE_MOTORS, DRIVE_PHOTOTAXIS) or mixed:
            # Kilobot._setup -> turn_left (kilobot.py:78-81, 315-316)
            self.motor_l = torch.full((E, N), 255, dtype=torch.uint8, device=dev)
            self.motor_r = torch.zeros(E, N, dtype=torch.uint8, device=dev)
        if drive_mode == DRIVE_PHOTOTAXIS or mixed:
            self.pt_threshold = torch.full((E, N), float('-inf'), dtype=torch.float32, device=dev)
            self.pt_update = torch.zeros(E, N, dtype=torch.int32, device=dev)
            self.pt_nochange = torch.zeros(E, N, dtype=torch.int32, device=dev)
            self.pt_dir = torch.zeros(E, N, dtype=torch.uint8, device=dev)
        self.light_vx = self.light_vy = None
        if light_type != LIGHT_NONE:
            LC = self._lib.kb_light_count(self._h)
            shape = (E,) if LC == 1 else (E, LC)
            self.light_x, self.light_y, self.light_vx, self.light_vy = f(*shape), f(*shape), f(*shape), f(*shape)
        cap = self._lib.kb_contact_capacity(self._h)
        self.ws_key = torch.zeros(E, cap, dtype=torch.int32, device=dev)
        self.ws_acc = f(E, cap)
        self.ws_cnt = torch.zeros(E, N, dtype=torch.uint8, device=dev)
        self.scratch = torch.empty(self._lib.kb_scratch_bytes(self._h), dtype=torch.uint8, device=dev)
        self.status = torch.zeros(E, dtype=torch.int32, device=dev)
        self._status_mask = None
        self.num_objects = M = self.cfg.num_objects
        self.ox = self.oy = self.otheta = self.ovx = self.ovy = self.ow = self.ows_acc = None
        if M > 0:
            self.ox, self.oy, self.otheta = f(E, M), f(E, M), f(E, M)
            self.ovx, self.ovy, self.ow = f(E, M), f(E, M), f(E, M)
            self.ows_acc = torch.full((E, nat.MAX_OBJECTS, nat.OWS_COLS, nat.OWS_WORDS), -1.0, dtype=torch.float32, device=dev)
        # sleeping (kb_config.allow_sleep): b2Body::m_sleepTime of every kilobot / object, < 0 = asleep
        self.sleep_time = self.osleep = None
        if self.cfg.allow_sleep:
            self.sleep_time = f(E, N)
            if M > 0:
                self.osleep = f(E, M)
        # IR-range neighbour sensing (kb_config.sense_radius): counts of the last substep's sensing point
        self.nbr_count = None
        if self.cfg.sense_radius > 0.0:
            self.nbr_count = torch.zeros(E, N, dtype=torch.int32, device=dev)
        self.light_value = self.light_gx = self.light_gy = None
        self.cmd_vx = self.cmd_vy = self.cmd_w = None
        if debug_outputs:
            self.light_value, self.light_gx, self.light_gy = f(E, N), f(E, N), f(E, N)
            self.cmd_vx, self.cmd_vy, self.cmd_w = f(E, N), f(E, N), f(E, N)
        self._bind()

    # ------------------------------------------------------------------ plumbing
    def _bind(self):
        b = nat.KbBuffers()
        for name in nat.BUFFER_FIELDS:
            t = getattr(self, name, None)
            setattr(b, name, None if t is None else t.data_ptr())
        self._call('kb_bind', C.byref(b), stream=False)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _call(self, name, *args, stream=True):
        """The library entry `name` on this sim's handle, with the current stream behind args unless stream=False; a failure
        raises under the entry's own name.  The launch goes to the CURRENT HIP device: make it the sim's."""
        with torch.cuda.device(self.device):
            if stream:
                args += (self._stream(),)
            nat.check(getattr(self._lib, name)(self._h, *args), name)

    def _mismatch(self, t, dtypes, shape, name):
        """What keeps t from being the tensor `name` -- contiguous, of one of dtypes, of this shape (an int: of at least
        that many elements), on the sim's device -- or None if nothing does."""
        least = isinstance(shape, int)
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype in dtypes and t.is_contiguous()
                and (t.numel() >= shape if least else tuple(t.shape) == tuple(shape))):
            dtypes = ' or '.join(dict.fromkeys(str(d).replace('torch.', '') for d in dtypes))
            return '%s must be a contiguous %s cuda tensor of %s' % (name, dtypes, 'at least %d elements' % shape if least else 'shape %s' % (tuple(shape),))
        if t.device != self.device:
            return '%s lives on %s, the simulator on %s' % (name, t.device, self.device)

    def _input(self, t, dtypes, shape, name, optional=False):
        """The pointer of a caller's tensor (None for None with optional=True); ValueError with what _mismatch says of it."""
        if t is None and optional:
            return None
        why = self._mismatch(t, dtypes, shape, name)
        if why:
            raise ValueError(why)
        return t.data_ptr()

    def close(self):
        if getattr(self, '_h', None) is not None and self._h:
            self._lib.kb_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def lds_bytes(self):
        return self._lib.kb_lds_bytes(self._h)

    @property
    def resident_envs_per_cu(self):
        """Workgroups (= envs) of this sim's kernel that one CU holds at a time (HIP occupancy query)."""
        with torch.cuda.device(self.device):
            n = self._lib.kb_resident_envs_per_cu(self._h)
        if n < 0:
            nat.check(n, 'kb_resident_envs_per_cu')
        return n

    @property
    def contact_capacity(self):
        return self._lib.kb_contact_capacity(self._h)

    @property
    def lds_staging_entries(self):
        """Contacts of one env that are staged in LDS (an env with more takes the global staging slice for that substep)."""
        return self._lib.kb_lds_staging_entries(self._h)

    @property
    def block_threads(self):
        return self._lib.kb_block_threads(self._h)

    @block_threads.setter
    def block_threads(self, n):
        self._call('kb_set_block_threads', int(n), stream=False)

    @property
    def variant_index(self):
        """Which instantiation of the step kernel runs this sim: its position in the library's list (kb_variant.h), -1 if
        the library has none.  Follows block_threads."""
        return self._lib.kb_variant_index(self._h)

    # ------------------------------------------------------------------ state
    def set_poses_m(self, xy_m, theta):
        """Body poses in metres / radians; stored as fp32 world units like body.py:32-34 does."""
        xy = np.asarray(xy_m, np.float64) * WORLD_SCALE
        self.x.copy_(torch.from_numpy(np.ascontiguousarray(xy[..., 0].astype(np.float32))).reshape(self.x.shape))
        self.y.copy_(torch.from_numpy(np.ascontiguousarray(xy[..., 1].astype(np.float32))).reshape(self.y.shape))
        self.theta.copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(theta, np.float32))).reshape(self.theta.shape))
        if self.sleep_time is not None:
            self.sleep_time.zero_()          # re-created bodies are awake
        self.forget_contacts()

    def forget_contacts(self):
        """Drop all warm-start impulses (bodies were re-created / teleported)."""
        self.ws_cnt.zero_()
        if self.ows_acc is not None:
            self.ows_acc.fill_(-1.0)

    def set_objects_m(self, xy_m, theta=None):
        """Object poses in metres / radians; objects start at rest (Body.__init__, body.py:32-38)."""
        xy = np.asarray(xy_m, np.float64) * WORLD_SCALE
        self.ox.copy_(torch.from_numpy(np.ascontiguousarray(xy[..., 0].astype(np.float32))).reshape(self.ox.shape))
        self.oy.copy_(torch.from_numpy(np.ascontiguousarray(xy[..., 1].astype(np.float32))).reshape(self.oy.shape))
        if theta is None:
            self.otheta.zero_()
        else:
            self.otheta.copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(theta, np.float32))).reshape(self.otheta.shape))
        self.ovx.zero_()
        self.ovy.zero_()
        self.ow.zero_()
        if self.osleep is not None:
            self.osleep.zero_()
        self.forget_contacts()

    def object_poses(self):
        """[num_envs, num_objects, 3] float32 (x [m], y [m], theta): get_state()['objects'] of every env."""
        # tensor / tensor: a true IEEE division like Body.get_pose (torch multiplies by the reciprocal for tensor / scalar)
        scale = torch.full_like(self.ox, WORLD_SCALE)
        return torch.stack([torch.div(self.ox, scale), torch.div(self.oy, scale), self.otheta], -1)

    def poses(self):
        """[num_envs, num_bots, 3] float32 (x [m], y [m], theta): get_state()['kilobots'] of every env."""
        out = torch.empty(self.num_envs, self.num_bots, 3, dtype=torch.float32, device=self.device)
        self._call('kb_get_poses', out.data_ptr())
        return out

    def host_state(self):
        """(kilobot poses [num_envs, num_bots, 3], object poses [num_envs, num_objects, 3], status [num_envs]) as numpy
        arrays, metres / radians: one launch and ONE copy to the host (kb_get_state), for get_state() after every step."""
        nat.refuse_capture('host_state()', 'call it outside the capture, or capture poses() and object_poses(), which stay on the device')
        N, M = self.num_bots, self.num_objects
        out = torch.empty(self.num_envs, 3 * (N + M) + 1, dtype=torch.float32, device=self.device)
        self._call('kb_get_state', out.data_ptr())
        h = out.cpu().numpy()
        E = self.num_envs
        return (h[:, :3 * N].reshape(E, N, 3), h[:, 3 * N:3 * (N + M)].reshape(E, M, 3),
                np.ascontiguousarray(h[:, -1]).view(np.int32))

    def status_bits(self):
        """OR of the status flags of all envs (one device read; synchronises the stream)."""
        nat.refuse_capture('status_bits()', "call it outside the capture (kb_buffers.status accumulates over the replays); an env takes on_status='ignore'")
        s = self.status
        if s.numel() <= (1 << 16):           # one small copy; OR on the host (4 reductions + 4 syncs cost 0.1 ms per env.step)
            return int(np.bitwise_or.reduce(s.cpu().numpy(), initial=0)) & sum(STATUS_BITS)
        if self._status_mask is None:
            self._status_mask = torch.tensor(sorted(STATUS_BITS), dtype=torch.int32, device=s.device)
        hit = (s.unsqueeze(-1) & self._status_mask).ne(0).any(0).cpu().numpy()
        return int(sum(b for b, h in zip(sorted(STATUS_BITS), hit) if h))

    def check_status(self, mode='raise', where=''):
        """Surface capacity overflows of the device step: mode 'raise' | 'warn' | 'ignore'.  Returns the bits."""
        if mode == 'ignore':
            return 0
        nat.refuse_capture('check_status(%r)' % (mode,), "call it outside the capture (kb_buffers.status accumulates over the replays), or with mode='ignore'")
        bits = self.status_bits()
        if bits:
            bad = int((self.status != 0).sum().item())
            nat.report_status(mode, where, bits, ' in %d of %d envs' % (bad, self.num_envs))
        return bits

    def sense(self, radius_m, out=None):
        """IR-range neighbour sensing on the current poses: [num_envs, num_bots] int32 counts of the kilobots within
        radius_m (centre to centre) of each kilobot (kb_sense; no reference counterpart)."""
        out, = self._outputs(out, [((self.num_envs, self.num_bots), torch.int32, 'count')], 'the count tensor')
        self._call('kb_sense', float(radius_m), out.data_ptr())
        return out

    def neighbors(self, radius_m, k, out=None, count=True):
        """Nearest-neighbour lists on the current poses (kb_sense_neighbors; no reference counterpart): for every kilobot the
        k nearest kilobots of its env within radius_m (centre to centre), ordered by distance, ties to the lower index.
        Returns (index [E, N, k] int32, -1 in unused slots; rel [E, N, k, 4] float32 = (metres ahead, metres to the left,
        distance in metres, heading of the neighbour minus the own heading), zeros in unused slots; count [E, N] int32 =
        kilobots in range, which may exceed k -- or None with count=False).  out: a tuple of preallocated contiguous
        tensors (index, rel[, count]) to write into."""
        E, N, k = self.num_envs, self.num_bots, int(k)
        if not 1 <= k <= nat.MAX_NEIGHBORS:
            raise ValueError('k must be in 1..%d' % nat.MAX_NEIGHBORS)
        shapes = [((E, N, k), torch.int32, 'index'), ((E, N, k, 4), torch.float32, 'rel')] + ([((E, N), torch.int32, 'count')] if count else [])
        out = self._outputs(out, shapes, 'a tuple of %d tensors (%s)' % (len(shapes), ', '.join(n for _, _, n in shapes)))
        out = tuple(out) + (() if count else (None,))
        self._call('kb_sense_neighbors', float(radius_m), k, *map(_ptr, out))
        return out

    def edges(self, radius_m, capacity=None, rel=True, src=True, out=None):
        """The whole IR-range graph on the current poses (kb_sense_edges; no reference counterpart): every pair of kilobots of
        an env within radius_m (centre to centre), both directions, as a CSR / COO edge list over the whole batch.  Kilobot i
        of env e is node e * num_bots + i; the row of a node holds its neighbours in ascending order.  Returns the named
        tuple Edges(src, dst, rel, offsets, count, nnz): src, dst [n] int32 node ids (src None with src=False), rel [n, 4]
        float32 as in neighbors() (None with rel=False), offsets [E * N + 1] int64 the CSR row pointer (the cumulative sum
        of count), count [E, N] int32 = sense(radius_m), nnz = offsets[-1], the number of edges.
        capacity=None: n = nnz, an int -- read from the device, the ONE synchronising read of this path; nnz == 0 gives
        empty tensors and still a valid offsets.  capacity=int: n = capacity, nothing is read back, nnz is a 0-dim int64
        tensor on the device for the caller to compare with capacity when it likes; edges behind the capacity are dropped
        from the end of the list, freshly allocated outputs hold -1 (src, dst) and 0 (rel) behind nnz.
        out: the preallocated contiguous tensors to write into, (src, dst, rel) without those switched off; slots behind
        nnz are left alone.  For an int64 edge_index [2, nnz] stack and cast in torch: torch.stack((src, dst)).long()."""
        E, N = self.num_envs, self.num_bots
        radius_m, capacity = nat.check_edges(radius_m, capacity)
        if capacity is None:
            nat.refuse_capture('edges(capacity=None)', 'pass capacity=int, which sizes the lists on the host and leaves nnz on the device')
        count = self.sense(radius_m)
        offsets = torch.zeros(E * N + 1, dtype=torch.int64, device=self.device)
        torch.cumsum(count.view(-1), 0, dtype=torch.int64, out=offsets[1:])
        nnz = offsets[-1]
        if capacity is None:
            nnz = int(nnz)          # the device read
        n = nnz if capacity is None else capacity
        shapes = ([((n,), torch.int32, 'src')] if src else []) + [((n,), torch.int32, 'dst')] + ([((n, 4), torch.float32, 'rel')] if rel else [])
        fresh = out is None
        out = list(self._outputs(out, shapes, 'a tuple of %d tensors (%s)' % (len(shapes), ', '.join(name for _, _, name in shapes))))
        if fresh and capacity is not None:
            for t, (_, _, name) in zip(out, shapes):
                t.fill_(0 if name == 'rel' else -1)
        t_src = out.pop(0) if src else None
        t_dst = out.pop(0)
        t_rel = out.pop(0) if rel else None
        self._sense_edges(radius_m, offsets, n, t_src, t_dst, t_rel, None)
        return Edges(t_src, t_dst, t_rel, offsets, count, nnz)

    def _sense_edges(self, radius_m, offsets, capacity, src, dst, rel, count):
        """The raw call of kb_sense_edges: offsets [E * N + 1] int64 as they are (the library clips what they say to the
        capacity), src / dst / rel / count contiguous tensors or None.  The sizes are checked here, because the library cannot:
        src, dst and rel hold at least `capacity` entries, offsets and count one per row."""
        rows, capacity = self.num_envs * self.num_bots, int(capacity)
        po, ps, pd, pr, pc = (self._input(t, dtypes, least, name, optional=True) for t, dtypes, least, name in (
            (offsets, I64, rows + 1, 'offsets'), (src, I32, capacity, 'src'), (dst, I32, capacity, 'dst'), (rel, F32, 4 * capacity, 'rel'), (count, I32, rows, 'count')))
        self._call('kb_sense_edges', float(radius_m), po, capacity, ps, pd, pr, pc)

    def neighbor_histogram(self, radius_m, n_rings, n_sectors, out=None, count=False):
        """Local neighbour histograms on the current poses (kb_sense_histogram; no reference counterpart): for every kilobot
        the number of kilobots of its env within radius_m (centre to centre), binned by distance (n_rings rings of equal
        width) and by bearing in its own frame (n_sectors sectors, sector 0 starting dead ahead, counter-clockwise).
        Returns hist [E, N, n_rings, n_sectors] float32, or (hist, count [E, N] int32 = kilobots in range = hist.sum((2, 3)))
        with count=True.  out: a preallocated contiguous hist tensor to write into (with count=True: the tuple (hist, count))."""
        E, N = self.num_envs, self.num_bots
        n_rings, n_sectors = nat.check_histogram_grid(n_rings, n_sectors)
        radius_m = nat.check_radius(radius_m)
        shapes = [((E, N, n_rings, n_sectors), torch.float32, 'hist')] + ([((E, N), torch.int32, 'count')] if count else [])
        out = self._outputs(out, shapes, 'the tuple (hist, count)' if count else 'the hist tensor')
        self._call('kb_sense_histogram', radius_m, n_rings, n_sectors, out[0].data_ptr(), out[1].data_ptr() if count else None)
        return (out[0], out[1]) if count else out[0]

    def neighbor_reduce(self, values, radius_m, op='sum', scale=65536.0, out=None, count=False):
        """IR-range message aggregation on the current poses (kb_sense_reduce; no reference counterpart): every kilobot
        broadcasts its row of `values` ([E, N] or [E, N, C] contiguous float32 on the sim's device, C <= 8) and hears, channel
        by channel, the op ('sum' | 'min' | 'max') over ALL kilobots of its env within radius_m (centre to centre).  The sum
        is a fixed-point sum of rint(values * scale) (clamped to +-2^21, NaN dropped) divided by scale: exact on the quantised
        values and independent of the order; the default scale resolves 1.5e-5 over +-32 per message.  min / max order the
        bit patterns (-0 < +0, NaNs outside the infinities) and return the value heard unchanged; scale is ignored.  Nothing
        heard: +0.0 / +inf / -inf.  Returns a tensor of the shape of values, or (result, count [E, N] int32 = kilobots
        heard) with count=True; the mean is result / count.  out: a preallocated tensor to write into, which may be values
        itself (with count=True: the tuple (result, count))."""
        E, N = self.num_envs, self.num_bots
        pv = self._input(values, F32, (E, N) + tuple(getattr(values, 'shape', ())[2:3]), 'values')
        op, n_channels, scale = nat.check_reduce(op, values.shape[2] if values.dim() == 3 else 1, scale)
        radius_m = nat.check_radius(radius_m)
        shapes = [(tuple(values.shape), torch.float32, 'result')] + ([((E, N), torch.int32, 'count')] if count else [])
        out = self._outputs(out, shapes, 'the tuple (result, count)' if count else 'the result tensor')
        self._call('kb_sense_reduce', radius_m, op, n_channels, scale, pv, out[0].data_ptr(), out[1].data_ptr() if count else None)
        return (out[0], out[1]) if count else out[0]

    def hops(self, seeds, radius_m, max_hops=None, parent=False, root=False, stats=False, out=None):
        """Hop-count gradients on the current poses (kb_sense_hops; no reference counterpart): for every kilobot the number of
        IR hops (edges of the graph of the kilobots within radius_m, centre to centre) to the nearest seed of its env, by one
        breadth-first search per env in one launch.  seeds: [E, N] bool or uint8, contiguous, on the sim's device; non-zero =
        seed.  Returns hops [E, N] int32: 0 at a seed, -1 where no seed is reachable within max_hops (None: no limit).
        parent=True adds parent [E, N] int32, the LOWEST-indexed neighbour one hop closer (-1 at seeds and where hops is -1);
        root=True root [E, N] int32, the seed at the end of the parent chain (-1 where hops is -1); stats=True stats [E, 2]
        int32 = (kilobots reached, seeds included; deepest hop, -1 without a seed).  With any of them the result is the tuple
        (hops, parent, root, stats) of the ones asked for.  out: the preallocated contiguous tensor(s) to write into, in the
        shape of the result."""
        E, N = self.num_envs, self.num_bots
        ps = self._input(seeds, MASK, (E, N), 'seeds')
        radius_m = nat.check_radius(radius_m)
        if max_hops is None:
            max_hops = nat.HOPS_UNLIMITED
        if isinstance(max_hops, bool) or not isinstance(max_hops, (int, np.integer)) or max_hops < 0:
            raise ValueError('max_hops must be a non-negative int or None')
        wanted = [True, bool(parent), bool(root), bool(stats)]
        shapes = [s for s, w in zip([((E, N), torch.int32, 'hops'), ((E, N), torch.int32, 'parent'), ((E, N), torch.int32, 'root'),
                                     ((E, 2), torch.int32, 'stats')], wanted) if w]
        out = list(self._outputs(out, shapes, 'the hops tensor' if len(shapes) == 1 else 'the tuple (%s)' % ', '.join(n for _, _, n in shapes)))
        given = iter(out)
        self._call('kb_sense_hops', radius_m, ps, min(int(max_hops), nat.HOPS_UNLIMITED), *(next(given).data_ptr() if w else None for w in wanted))
        return tuple(out) if len(out) > 1 else out[0]

    def clusters(self, radius_m, select=None, size=False, table=False, stats=False, out=None):
        """Connected components of the IR-range graph on the current poses (kb_sense_clusters; no reference counterpart):
        which kilobots hang together through edges of at most radius_m, centre to centre, by one union-find per env in one
        launch.  Returns label [E, N] int32: the LOWEST index of the kilobot's component.  select: [E, N] bool or uint8 on the
        sim's device, the kilobots that are in the graph (None: all); one that is not has label -1 and connects nothing.
        size=True adds size [E, N] int32, the kilobots in the component (0 where label is -1); table=True table [E, N, 4]
        float32, row r = (size, centroid x, centroid y, distance of the farthest member from the centroid), metres in the world
        frame, of the component whose label is r and zeros in every other row -- a kilobot's own row is table[e, label] --, from
        fixed-point sums at 2^-16 world units that do not depend on the order; stats=True stats [E, 4] int32 = (components, size
        of the largest, its label with ties to the lowest and -1 without a kilobot, components of one).  stats[:, 1] / N is the
        aggregation metric.  With any of them the result is the tuple (label, size, table, stats) of the ones asked for.  out:
        the preallocated contiguous tensor(s) to write into, in the shape of the result; every element is written."""
        E, N = self.num_envs, self.num_bots
        radius_m = nat.check_radius(radius_m)
        ps = self._input(select, MASK, (E, N), 'select', optional=True)
        wanted = [True, bool(size), bool(table), bool(stats)]
        shapes = [s for s, w in zip([((E, N), torch.int32, 'label'), ((E, N), torch.int32, 'size'), ((E, N, 4), torch.float32, 'table'),
                                     ((E, 4), torch.int32, 'stats')], wanted) if w]
        out = list(self._outputs(out, shapes, 'the label tensor' if len(shapes) == 1 else 'the tuple (%s)' % ', '.join(n for _, _, n in shapes)))
        given = iter(out)
        parts = [next(given) if w else None for w in wanted]
        if parts[2] is not None and parts[2].data_ptr() % 16:
            raise ValueError('out: table must be 16-byte aligned')
        self._call('kb_sense_clusters', radius_m, ps, *map(_ptr, parts))
        return tuple(out) if len(out) > 1 else out[0]

    def outline(self):
        """The geometry object_points() reads (kb_get_outline) as a KbOutline: the arena bounds and the fixtures grouped by
        body in stable order -- the order that decides ties -- in world units."""
        return nat.outline(self._h)

    def object_points(self, out=None, walls=True):
        """Object and wall points on the current poses (kb_sense_objects; no reference counterpart): for every kilobot the
        nearest point of every object of its env and of the arena walls, in its own frame.  Returns (obj [E, N, M, 4], wall
        [E, N, 4]) float32: obj = (metres ahead, metres to the left, distance in metres, 1.0 if the kilobot's centre is inside
        the object else 0.0), one row per object in object order, no range cut; wall = (metres ahead, metres to the left,
        signed distance in metres -- negative outside the arena --, index of the wall: 0 = xmin, 1 = xmax, 2 = ymin, 3 = ymax).
        With the centre inside an object the point is the nearest fixture edge, which on an LForm / TForm / CForm may be an
        interior edge.  walls=False returns obj alone; a sim without objects returns wall alone, and raises ValueError with
        walls=False.  out: the preallocated contiguous tensor(s) to write into, in the shape of the result."""
        E, N, M = self.num_envs, self.num_bots, self.num_objects
        if M == 0 and not walls:
            raise ValueError('object_points(walls=False) asks for object points, but the sim has no objects')
        shapes = ([((E, N, M, 4), torch.float32, 'obj')] if M > 0 else []) + ([((E, N, 4), torch.float32, 'wall')] if walls else [])
        out = self._outputs(out, shapes, 'the tuple (obj, wall)' if len(shapes) == 2 else 'the %s tensor' % shapes[0][2])
        if any(t.data_ptr() % 16 for t in out):
            raise ValueError('out: the tensors must be 16-byte aligned')
        self._call('kb_sense_objects', out[0].data_ptr() if M > 0 else None, out[-1].data_ptr() if walls else None)
        return out if len(out) == 2 else out[0]

    def grid_channels(self, planes=('count',)):
        """The channels of occupancy_grid() for these planes (kb_grid_channels): 1 for 'count', 2 for 'flow', one per object
        for 'objects'.  ValueError for 'objects' on a sim without objects."""
        planes = nat.check_grid(1, 1, planes)[2]
        if planes & nat.GRID_OBJECTS and self.num_objects == 0:
            raise ValueError("planes: 'objects' asked for, but the sim has no objects")
        n = self._lib.kb_grid_channels(self._h, planes)
        if n < 0:
            nat.check(n, 'kb_grid_channels')
        return n

    def occupancy_grid(self, width, height, planes=('count',), out=None):
        """Top-down occupancy grids on the current poses (kb_sense_grid; no reference counterpart): the arena of every env cut
        into width x height equal cells, row 0 at ymin and column 0 at xmin -- the fixed-size image of the table a central
        policy is fed.  planes: a GRID_* mask or an iterable of 'count' (1 channel: kilobots in the cell), 'flow' (2 channels:
        the sums of cos(theta) and of sin(theta) over the kilobots in the cell, fixed-point sums at 2^-16 that do not depend on
        the order) and 'objects' (one channel per object: 1.0 where the cell centre is inside the object); the channels come in
        that order.  A kilobot outside the arena counts in the nearest edge cell.  Returns [E, C, height, width] float32 on the
        sim's device.  out: a preallocated contiguous tensor of that shape to write into; every element is written."""
        width, height, planes = nat.check_grid(width, height, planes)
        channels = self.grid_channels(planes)
        out, = self._outputs(out, [((self.num_envs, channels, height, width), torch.float32, 'grid')], 'the grid tensor')
        self._call('kb_sense_grid', width, height, planes, out.data_ptr())
        return out

    def coverage(self, width, height, select=None, owner=True, dist=True, cells=True, stats=True, out=None):
        """Nearest-kilobot fields on the current poses (kb_sense_coverage; no reference counterpart): the arena of every env
        cut into width x height cells as in occupancy_grid(), and for every cell centre the nearest kilobot of the env -- the
        Voronoi partition of the table on this grid.  Returns the named tuple Coverage(owner, dist, cells, stats): owner
        [E, height, width] int32, the index of the nearest kilobot (ties to the lower index); dist [E, height, width] float32,
        its distance in metres; cells [E, N, 4] float32, the Voronoi cell of every kilobot as (centroid metres ahead, centroid
        metres to the left, area in grid cells, largest distance of one of its cell centres in metres) -- the first two are
        the step of Lloyd's coverage control in the kilobot's own frame --, zeros for a kilobot that owns nothing; stats
        [E, 2] float32 = (the sum over the cells of the squared distance in square metres, a fixed-point sum at 2^-16 world
        units squared that does not depend on the order; the distance of the worst-covered cell centre in metres).  A part
        switched off (owner=False, ...) is None and is not computed; at least one must be on.  select: [E, N] bool or uint8
        on the sim's device, the kilobots that take part (None: all); an env that selects none has owner -1, dist and stats
        +inf.  out: the preallocated contiguous tensors to write into, a tuple of the parts that are on; every element is
        written."""
        E, N = self.num_envs, self.num_bots
        width, height = nat.check_coverage(width, height)
        wanted = [bool(owner), bool(dist), bool(cells), bool(stats)]
        if not any(wanted):
            raise ValueError('coverage: at least one of owner, dist, cells and stats must be on')
        ps = self._input(select, MASK, (E, N), 'select', optional=True)
        shapes = [s for s, w in zip([((E, height, width), torch.int32, 'owner'), ((E, height, width), torch.float32, 'dist'),
                                     ((E, N, 4), torch.float32, 'cells'), ((E, 2), torch.float32, 'stats')], wanted) if w]
        given = iter(self._outputs(out, shapes, 'the tensor' if len(shapes) == 1 else 'the tuple (%s)' % ', '.join(n for _, _, n in shapes)))
        parts = [next(given) if w else None for w in wanted]
        if parts[2] is not None and parts[2].data_ptr() % 16:
            raise ValueError('out: cells must be 16-byte aligned')
        self._call('kb_sense_coverage', width, height, ps, *map(_ptr, parts))
        return Coverage(*parts)

    def new_field(self, width, height, channels=1):
        """A pheromone field for field_step(): zeros [E, channels, height, width] float32 on the sim's device.  The caller owns
        it; the sim keeps nothing of it."""
        width, height, channels = nat.check_field(width, height, channels, 1.0, 0.0, 0)[:3]
        return torch.zeros(self.num_envs, channels, height, width, dtype=torch.float32, device=self.device)

    def field_step(self, field, amount=None, keep=1.0, spread=0.0, iters=1, env_mask=None, sense=True, out=None):
        """One update of a pheromone field on the current poses, IN PLACE and in one launch (kb_field_step; no reference
        counterpart): field [E, C, height, width] contiguous float32 on the sim's device (new_field) lies over the arena like
        occupancy_grid(), row 0 at ymin and column 0 at xmin.  Deposit: kilobot i adds amount[e, i, c] to the cell it stands in
        -- amount [E, N, C] or, with one channel, [E, N]; a fixed-point sum at 2^-16 of amounts clamped to +-16 that does not
        depend on the order, NaN counts as 0; None deposits nothing.  Then `iters` times u' = keep * (u + spread * lap(u)) with
        the 5-point Laplacian and zero-flux edges: keep in [0, 1] (1 = no decay) and spread in [0, 0.25], a number or one per
        channel.  Then every kilobot reads the field at its cell: returns sense [E, N, C, 4] float32 = (value, gradient per
        metre ahead, gradient per metre to the left, what the cell received in this call), or None with sense=False.
        env_mask: [E] bool or uint8 on the sim's device; of the envs it does not select no byte of field or sense is written.
        amount=None with iters=0 is a pure read that leaves field untouched.  out: the preallocated contiguous sense tensor."""
        E, N = self.num_envs, self.num_bots
        if not torch.is_tensor(field) or field.dim() != 4:
            raise ValueError('field must be a contiguous float32 cuda tensor of shape (%d, channels, height, width)' % E)
        C_, height, width = (int(s) for s in field.shape[1:])
        width, height, C_, keep, spread, iters = nat.check_field(width, height, C_, keep, spread, iters)
        pf = self._input(field, F32, (E, C_, height, width), 'field')
        one = C_ == 1 and torch.is_tensor(amount) and amount.dim() == 2
        pa = self._input(amount, F32, (E, N) if one else (E, N, C_), 'amount', optional=True)
        pm = self._input(env_mask, MASK, (E,), 'env_mask', optional=True)
        if sense:
            out, = self._outputs(out, [((E, N, C_, 4), torch.float32, 'sense')], 'the sense tensor')
            if out.data_ptr() % 16:
                raise ValueError('out: sense must be 16-byte aligned')
        elif out is not None:
            raise ValueError('out given with sense=False')
        elif amount is None and iters == 0:
            raise ValueError('field_step: nothing to do (amount=None, iters=0 and sense=False)')
        vec = C.c_float * C_
        self._call('kb_field_step', width, height, C_, vec(*keep), vec(*spread), iters, pm, pa, pf, _ptr(out))
        return out

    def targets(self, points_m, tol_m, bot_select=None, slot_select=None, index=True, rel=True, owner=True, dist=True, stats=True, out=None,
                match='nearest', cutoff_m=None):
        """Kilobot-to-slot matching on the current poses (kb_sense_targets; no reference counterpart): the two-sided nearest
        query of shape formation between the kilobots of every env and the K points ("slots") of a target shape.  points_m:
        contiguous float32 [E, K, 2] or [K, 2] (shared by all envs) on the sim's device, metres, 1 <= K <= MAX_TARGETS.
        Returns the named tuple Targets(index, rel, owner, dist, stats): index [E, N] int32, the slot nearest to every
        kilobot (ties to the lower index); rel [E, N, 4] float32 = (that slot metres ahead, metres to the left, its distance in
        metres, 1.0 if the kilobot is also the one nearest to that slot) in the kilobot's own frame; owner [E, K] int32, the
        kilobot nearest to every slot (ties to the lower index); dist [E, K] float32, its distance in metres -- a slot is
        free while that is large; stats [E, 6] float32 = (the sum over the kilobots of the squared distance to their slot in
        square metres, the largest such distance in metres, the same two over the slots to their owners -- the directed
        Chamfer sums, fixed-point sums that do not depend on the order, and Hausdorff distances --, the number of slots whose
        owner is within tol_m, the number of kilobots whose slot is within tol_m).  bot_select [E, N] and slot_select [E, K],
        bool or uint8 on the sim's device, restrict the two sides (None: all): what is not selected gets -1 and zeros, a
        selected entry of an env whose other side is empty -1 and a distance of +inf, and the stats of such an env are
        (+inf, +inf, +inf, +inf, 0, 0).  A part switched off (index=False, ...) is None and is not computed; at least one
        must be on.  out: the preallocated contiguous tensors to write into, a tuple of the parts that are on; every element
        is written.
        match='greedy' (kb_sense_assign) returns a ONE-TO-ONE matching in the same tuple instead of the two nearest queries:
        of all pairs of a selected kilobot and a selected slot no further apart than cutoff_m (metres; None: no limit), in
        ascending order of (distance, kilobot, slot), a pair is taken iff neither end has been taken -- the greedy matching,
        on the device in one launch.  index is then the slot matched to a kilobot or -1, rel its row with a fourth word of 1.0
        (an unmatched selected kilobot: (0, 0, +inf, 0)), owner and dist the kilobot matched to a slot and its distance (an
        unmatched selected slot: -1 and +inf), and stats = (the sum of the squared distances of the matched pairs in square
        metres, the largest distance, the sum of the distances in metres, the number of rounds of mutual choices the
        matching takes, the number of pairs within tol_m, the number of pairs); all zero in an env without a pair."""
        E, N = self.num_envs, self.num_bots
        if match not in ('nearest', 'greedy'):
            raise ValueError("match must be 'nearest' or 'greedy'")
        if match == 'nearest' and cutoff_m is not None:
            raise ValueError("cutoff_m needs match='greedy'")
        if not torch.is_tensor(points_m) or points_m.dim() not in (2, 3):
            raise ValueError('points_m must be a contiguous float32 cuda tensor of shape (E, K, 2) or (K, 2)')
        if match == 'greedy':
            K, tol_m, cutoff_m = nat.check_assign(points_m.shape[-2], tol_m, cutoff_m)
        else:
            K, tol_m = nat.check_targets(points_m.shape[-2], tol_m)
        per_env = points_m.dim() == 3
        pp = self._input(points_m, F32, (E, K, 2) if per_env else (K, 2), 'points_m')
        wanted = [bool(index), bool(rel), bool(owner), bool(dist), bool(stats)]
        if not any(wanted):
            raise ValueError('targets: at least one of index, rel, owner, dist and stats must be on')
        pb = self._input(bot_select, MASK, (E, N), 'bot_select', optional=True)
        ps = self._input(slot_select, MASK, (E, K), 'slot_select', optional=True)
        shapes = [s for s, w in zip([((E, N), torch.int32, 'index'), ((E, N, 4), torch.float32, 'rel'), ((E, K), torch.int32, 'owner'),
                                     ((E, K), torch.float32, 'dist'), ((E, 6), torch.float32, 'stats')], wanted) if w]
        given = iter(self._outputs(out, shapes, 'the tensor' if len(shapes) == 1 else 'the tuple (%s)' % ', '.join(n for _, _, n in shapes)))
        parts = [next(given) if w else None for w in wanted]
        if parts[1] is not None and parts[1].data_ptr() % 16:
            raise ValueError('out: rel must be 16-byte aligned')
        if match == 'greedy':
            self._call('kb_sense_assign', pp, K, int(per_env), tol_m, cutoff_m, pb, ps, *map(_ptr, parts))
        else:
            self._call('kb_sense_targets', pp, K, int(per_env), tol_m, pb, ps, *map(_ptr, parts))
        return Targets(*parts)

    def path_costs(self, width, height):
        """The integer step costs (qx, qy, qd) of paths() on a width x height grid (kb_path_costs): a move along x, along y and
        along a diagonal in 1/1024 world units, i.e. 1 / 25600 metres.  Host only."""
        width, height = nat.check_paths(width, height)[:2]
        q = (C.c_int32 * 3)()
        nat.check(self._lib.kb_path_costs(self._h, width, height, q), 'kb_path_costs')
        return tuple(q)

    def path_cells(self, points_m, width, height):
        """The uint8 mask [E, height, width] of the cells of the width x height grid that points in metres fall in: points_m
        array-like or tensor [E, K, 2] or [K, 2] (shared by all envs), binned on the host by the grid's cell rule
        (nat.path_cells: a point outside the arena lands in the nearest edge cell) and uploaded.  What lets the goal of
        paths() be given as positions; not for the inner loop."""
        nat.refuse_capture('path_cells()', 'it bins the points on the host and uploads the mask; call it before the capture and write into the mask in place')
        points = np.asarray(points_m.cpu() if torch.is_tensor(points_m) else points_m, dtype=np.float32)
        if points.ndim == 3 and points.shape[0] != self.num_envs:
            raise ValueError('points_m must have the shape (K, 2) or (%d, K, 2)' % self.num_envs)
        mask = nat.path_cells(self.outline().arena, points, width, height)
        return torch.from_numpy(np.broadcast_to(mask, (self.num_envs, height, width)).copy(order='C')).to(self.device)

    def paths(self, width, height, source, blocked=None, objects='all', clearance_m=0.0, dist=True, step=True, bots=True, stats=True, out=None):
        """Obstacle-aware distance-to-goal fields on the current poses (kb_sense_paths; no reference counterpart): the arena of
        every env cut into width x height cells as in occupancy_grid(), and for every cell the length of the shortest
        8-connected path to the nearest cell of `source` that crosses no blocked cell and cuts no corner.  source, blocked:
        [E, height, width] bool or uint8 on the sim's device (path_cells() makes one from positions); blocked None blocks
        nothing.  objects: which objects of the sim block as well -- 'all', a mask or an iterable of object indices (0 or ():
        none); a cell is blocked where its centre is inside the object or, with clearance_m > 0, within clearance_m of its
        outline (a kilobot radius keeps the path wide enough for a kilobot).  Returns the named tuple Paths(dist, step, bots,
        stats): dist [E, height, width] float32, metres to go, +inf where blocked or cut off; step [E, height, width] int8, the
        direction 0..7 of the next cell (counter-clockwise from +x in steps of 45 degrees), -1 at a goal cell, -2 where cut
        off, -3 where blocked; bots [E, N, 4] float32 = (metres to go from the kilobot's cell, the unit vector of the next move
        ahead and to the left in the kilobot's own frame, flag: 0 on a free reached cell, 1 on a goal cell, 2 on a blocked cell
        with a free reached neighbour -- the normal case for a kilobot pressing on an object: it gets the best way out --, 3
        unreachable with +inf and a zero direction); stats [E, 4] float32 = (kilobots that can reach the goal, the sum of their
        metres to go, the largest of them, free cells reached).  All distances are integer sums: nothing depends on any
        order.  A part switched off (dist=False, ...) is None and is not computed; at least one must be on.  out: the
        preallocated contiguous tensors to write into, a tuple of the parts that are on; every element is written."""
        E, N = self.num_envs, self.num_bots
        width, height, clearance_m = nat.check_paths(width, height, clearance_m)
        objects = nat.check_path_objects(objects, self.num_objects)
        wanted = [bool(dist), bool(step), bool(bots), bool(stats)]
        if not any(wanted):
            raise ValueError('paths: at least one of dist, step, bots and stats must be on')
        ps = self._input(source, MASK, (E, height, width), 'source')
        pb = self._input(blocked, MASK, (E, height, width), 'blocked', optional=True)
        shapes = [s for s, w in zip([((E, height, width), torch.float32, 'dist'), ((E, height, width), torch.int8, 'step'),
                                     ((E, N, 4), torch.float32, 'bots'), ((E, 4), torch.float32, 'stats')], wanted) if w]
        given = iter(self._outputs(out, shapes, 'the tensor' if len(shapes) == 1 else 'the tuple (%s)' % ', '.join(n for _, _, n in shapes)))
        parts = [next(given) if w else None for w in wanted]
        if parts[2] is not None and parts[2].data_ptr() % 16:
            raise ValueError('out: bots must be 16-byte aligned')
        self._call('kb_sense_paths', width, height, ps, pb, objects, clearance_m, *map(_ptr, parts))
        return Paths(*parts)

    def contacts(self, k=8, scale=65536.0, out=None):
        """Touch and push sensing from the contact store of the last step (kb_sense_contacts; Body.collides_with of every
        kilobot at once, with the impulses the solver applied): returns (partner, impulse, touch, obj).  partner [E, N, k]
        int32 and impulse [E, N, k] float32: the first k contacts of every kilobot -- a kilobot j < N, wall N + w (w: 0 = xmin,
        1 = xmax, 2 = ymin, 3 = ymax as in object_points) or object N + 4 + m, in that order, one entry per fixture of an
        object -- with the accumulated normal impulse in Box2D world units; -1 and 0.0 in unused slots.  touch [E, N, 4]
        float32: kilobot contacts, wall contacts, fixture contacts and the impulse sum over ALL contacts of the kilobot,
        whatever k.  obj [E, M, 2] float32: the kilobot contacts on every object and their impulse sum; None without objects.
        The sums are fixed-point sums of rint(impulse * scale) divided by scale, as in neighbor_reduce: independent of the
        order.  k=0 skips the lists: partner and impulse are None.  The contacts are those the last world step found (on
        the poses before its integration); forget_contacts() empties them.  out: a tuple of the preallocated contiguous
        tensors that are returned (None left out) to write into."""
        E, N, M, k = self.num_envs, self.num_bots, self.num_objects, int(k)
        if not 0 <= k <= nat.MAX_CONTACT_SLOTS:
            raise ValueError('k must be in 0..%d' % nat.MAX_CONTACT_SLOTS)
        scale = float(scale)
        if not 0.0 < scale < float('inf'):
            raise ValueError('scale must be finite and positive')
        shapes = ([((E, N, k), torch.int32, 'partner'), ((E, N, k), torch.float32, 'impulse')] if k else []) \
            + [((E, N, 4), torch.float32, 'touch')] + ([((E, M, 2), torch.float32, 'obj')] if M > 0 else [])
        out = list(self._outputs(out, shapes, 'a tuple of %d tensors (%s)' % (len(shapes), ', '.join(n for _, _, n in shapes))))
        partner, impulse = (out.pop(0), out.pop(0)) if k else (None, None)
        touch, obj = out[0], out[1] if M > 0 else None
        self._call('kb_sense_contacts', k, scale, _ptr(partner), _ptr(impulse), _ptr(touch), _ptr(obj))
        return partner, impulse, touch, obj

    def render(self, width, height, layers=('objects', 'bots', 'light'), style=None, body_rgb=None, mark_rgb=None, out=None):
        """RGB frames of every env on the current state (kb_render; KilobotsEnv.render of the reference as a point-sampled
        image, include/kilobots_hip.h): [E, height, width, 3] uint8 on the sim's device, row 0 at ymax, column 0 at xmin.
        layers: a RENDER_* mask or an iterable of 'objects', 'bots' and 'light', painted in that order; 'objects' on a sim
        without objects and 'light' on a sim without a positional light draw nothing.  style: a dict of the fields of
        kb_render_style ('table', 'body', 'ring', 'mark', 'light': (R, G, B); 'light_alpha'; 'obj': a list of colours, one per
        object); missing keys take the reference's colours.  body_rgb, mark_rgb: contiguous int32 / uint32 tensors [E, N] of
        0x00RRGGBB words on the sim's device, the body colour and the colour of the heading mark of every kilobot; None: the
        style's.  out: a preallocated contiguous uint8 tensor of the result's shape to write into; every byte is written."""
        width, height, layers = nat.check_render(width, height, layers)
        st = style if isinstance(style, nat.KbRenderStyle) else nat.render_style(style)
        out, = self._outputs(out, [((self.num_envs, height, width, 3), torch.uint8, 'rgb')], 'the rgb tensor')
        pb, pm = (self._input(t, WORD, (self.num_envs, self.num_bots), name, optional=True) for name, t in (('body_rgb', body_rgb), ('mark_rgb', mark_rgb)))
        self._call('kb_render', width, height, layers, C.byref(st), pb, pm, out.data_ptr())
        return out

    def rays(self, radius_m, n_rays, targets=None, out=None, hit=True):
        """Range scans on the current poses (kb_sense_rays; no reference counterpart): for every kilobot and each of n_rays
        bearings in its own frame (ray 0 dead ahead, counter-clockwise, nat.ray_directions) how far the first thing in that
        direction is, up to radius_m, and what it is.  Returns (dist [E, N, n_rays] float32: metres, radius_m where nothing was
        hit; hit [E, N, n_rays] int32: a kilobot j < N, wall N + w (w: 0 = xmin, 1 = xmax, 2 = ymin, 3 = ymax as in
        object_points) or object N + 4 + m -- the codes of contacts() --, -1 where nothing was hit; None with hit=False).  A
        body hidden behind another is not seen; a kilobot inside a body sees the way out.  targets: a RAY_* mask or an
        iterable of 'bots', 'objects' and 'walls'; None: everything the sim has ('objects' only with objects).  out: the
        preallocated contiguous tensors to write into, the tuple (dist, hit), or dist alone with hit=False; every element is
        written."""
        E, N = self.num_envs, self.num_bots
        if targets is None:
            targets = nat.RAY_BOTS | nat.RAY_WALLS | (nat.RAY_OBJECTS if self.num_objects > 0 else 0)
        radius_m, n_rays, targets = nat.check_rays(radius_m, n_rays, targets)
        if targets & nat.RAY_OBJECTS and self.num_objects == 0:
            raise ValueError("targets: 'objects' asked for, but the sim has no objects")
        shapes = [((E, N, n_rays), torch.float32, 'dist')] + ([((E, N, n_rays), torch.int32, 'hit')] if hit else [])
        out = self._outputs(out, shapes, 'the tuple (dist, hit)' if hit else 'the dist tensor')
        self._call('kb_sense_rays', radius_m, n_rays, targets, out[0].data_ptr(), out[1].data_ptr() if hit else None)
        return out[0], out[1] if hit else None

    def _outputs(self, out, shapes, what):
        """The outputs of a sensing call as a tuple: `out` checked against shapes = [(shape, dtype, name), ...] (a lone
        tensor counts as a tuple of one), or freshly allocated if out is None.  what: how a message names the whole."""
        if out is None:
            return tuple(torch.empty(*s, dtype=d, device=self.device) for s, d, _ in shapes)
        out = (out,) if torch.is_tensor(out) else tuple(out)
        if len(out) != len(shapes):
            raise ValueError('out must be %s' % what)
        for t, (s, d, n) in zip(out, shapes):
            why = self._mismatch(t, (d,), s, 'out: ' + n)
            if why:
                raise ValueError(why)
        return out

    def light_sense(self, light_action=None):
        """The sensing point of one substep on its own (kb_light_sense): Light.step with `light_action` (None: the light
        stays) + value_and_gradients at every kilobot's sensor into light_value / light_gx / light_gy -- for kilobots whose
        _loop runs on the host between the sensing and the motor law (kilobots_env.py:171-184)."""
        if self.light_value is None:
            raise ValueError('light_sense needs the sensing outputs: create the sim with debug_outputs=True')
        self._call('kb_light_sense', self._light_action_ptr(light_action))

    def reset(self, seed=0, mean=(0.0, 0.0), std=0.1, random_theta=False, random_velocity=False, resolve=True, env_offset=0):
        """KilobotsEnv.reset of every env on the device (kb_reset): Gaussian spawn clipped to the bounds -/+ 0.02 m
        (yaml_kilobots_env.py:346-352), Philox4x32-10 keyed by (seed; env_offset + env, bot), then the step to resolve."""
        self._call('kb_reset', C.byref(_reset_params(seed, mean, std, random_theta, random_velocity, resolve, env_offset)))

    # ------------------------------------------------------------------ stepping
    def _actions_ptr(self, actions):
        return self._input(actions, F32, (self.num_envs, self.num_bots, 2), 'actions', optional=True)

    def _light_action_ptr(self, light_action):
        return self._input(light_action, F32, (self.num_envs, self._lib.kb_light_action_dim(self._h)), 'light_action', optional=True)

    def set_actions(self, actions):
        """set_action of every kilobot (clamped); actions [E, N, 2] cuda float32 or None (= zeros)."""
        self._call('kb_set_actions', self._actions_ptr(actions))

    def step(self, n_substeps=1, actions=None, light_action=None, flags=0, env_mask=None):
        """n_substeps iterations of the reference substep loop in one kernel launch (asynchronous).
        env_mask: [E] bool or uint8 tensor on the sim's device: only the envs it selects are stepped (kb_step_envs); of the
        others no byte of any state tensor changes, the fused actions included.  None: every env (kb_step)."""
        args = self._actions_ptr(actions), self._light_action_ptr(light_action), int(n_substeps), int(flags)
        if env_mask is None:
            self._call('kb_step', *args)
        else:
            self._call('kb_step_envs', self._input(env_mask, MASK, (self.num_envs,), 'env_mask'), *args)

    def reset_envs(self, env_mask, seed=0, mean=(0.0, 0.0), std=0.1, random_theta=False, random_velocity=False, resolve=True, env_offset=0,
                   episode=None, objects=None, lights=None, light_vel=None):
        """KilobotsEnv.reset of the envs env_mask selects ([E] bool or uint8 on the sim's device), on the device and without a
        host synchronisation (kb_reset_envs): the spawn of reset() for those envs, then the step to resolve for them alone.  Of
        the other envs no byte of any state tensor changes.
        episode: [E] int32 -- word z of the Philox counter (env_offset + env, bot, z, 0) of every env; None: 0, the draw of
        reset().  Counting the episodes of every env there gives each of its episodes a spawn of its own.
        objects: [E, M, 3] float32 (ox, oy in world units as stored, otheta): the selected envs' objects are put there at rest.
        lights, light_vel: [E, L, 2] float32 (or [E, 2] with one light): light_x, light_y and light_vx, light_vy of the selected
        envs; with lights alone the velocities are zeroed.  All tensors contiguous and on the sim's device."""
        E, M = self.num_envs, self.num_objects
        rp = _reset_params(seed, mean, std, random_theta, random_velocity, resolve, env_offset)
        if objects is not None and M == 0:
            raise ValueError('objects given, but the sim has no objects')
        if (lights is not None or light_vel is not None) and self.light_x is None:
            raise ValueError('lights / light_vel given, but the sim has no light')
        light_shape = None if self.light_x is None else tuple(self.light_x.shape) + (2,)
        init = nat.KbEpisodeInit(self._input(episode, WORD, (E,), 'episode', optional=True), self._input(objects, F32, (E, M, 3), 'objects', optional=True),
                                 self._input(lights, F32, light_shape, 'lights', optional=True), self._input(light_vel, F32, light_shape, 'light_vel', optional=True))
        self._call('kb_reset_envs', C.byref(rp), self._input(env_mask, MASK, (E,), 'env_mask'), C.byref(init))
