"""ctypes binding of libkilobots_hip.so (include/kilobots_hip.h).

The library is the product: there is no CPU fallback.  If it is missing this module raises
ImportError-like RuntimeError at load() time with the build command.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('KB_HIP_LIB', os.path.join(HERE, 'libkilobots_hip.so'))

KB_OK, KB_EINVAL, KB_ENOTBOUND, KB_EHIP, KB_ELDS = 0, -1, -2, -3, -4
DRIVE_VELOCITY, DRIVE_ACCEL, DRIVE_MOTORS, DRIVE_SIMPLE_PHOTOTAXIS, DRIVE_PHOTOTAXIS, DRIVE_MIXED = range(6)
LIGHT_NONE, LIGHT_CIRCULAR, LIGHT_GRADIENT, LIGHT_MOMENTUM, LIGHT_COMPOSITE = range(5)
MAX_LIGHTS = 4
STEP_NO_DRIVE = 1
MAX_OBJECTS = 8
MAX_POLY_VERTS = 4
SHAPE_CIRCLE, SHAPE_BOX, SHAPE_POLYGON = range(3)
OWS_COLS, OWS_WORDS = 12, 6
MAX_BOTS = 1024
MAX_NEIGHBORS = 16     # KB_MAX_NEIGHBORS: slots per kilobot of kb_sense_neighbors
HIST_MAX_RINGS, HIST_MAX_SECTORS, HIST_MAX_BINS = 8, 16, 64     # KB_HIST_MAX_*: bin grid of kb_sense_histogram
REDUCE_SUM, REDUCE_MIN, REDUCE_MAX = range(3)     # kb_reduce_op: how kb_sense_reduce combines the messages heard
REDUCE_MAX_CHANNELS = 8     # KB_REDUCE_MAX_CHANNELS: floats per message of kb_sense_reduce
HOPS_UNLIMITED = MAX_BOTS     # KB_HOPS_UNLIMITED: the max_hops of kb_sense_hops that cuts nothing
GRID_COUNT, GRID_FLOW, GRID_OBJECTS = 1, 2, 4     # KB_GRID_*: the planes of kb_sense_grid, a bit each
MAX_CONTACT_SLOTS = 16     # KB_MAX_CONTACT_SLOTS: slots per kilobot of kb_sense_contacts
GRID_MAX_SIDE = 128     # KB_GRID_MAX_SIDE: cells along either side of the grid of kb_sense_grid
MAX_TARGETS = 1024     # KB_MAX_TARGETS: slots of the target shape of kb_sense_targets
FIELD_MAX_CHANNELS, FIELD_MAX_ITERS = 4, 64     # KB_FIELD_MAX_*: channels of a field and iterations per call of kb_field_step
RENDER_OBJECTS, RENDER_BOTS, RENDER_LIGHT = 1, 2, 4     # KB_RENDER_*: the layers of kb_render, a bit each
RENDER_MAX_SIDE = 2048     # KB_RENDER_MAX_SIDE: pixels along either side of a frame of kb_render
RAY_BOTS, RAY_OBJECTS, RAY_WALLS = 1, 2, 4     # KB_RAY_*: what the rays of kb_sense_rays can hit, a bit each
MAX_RAYS = 32     # KB_MAX_RAYS: rays per kilobot of kb_sense_rays
DAMPING_PADE, DAMPING_LINEAR = 0, 1
WORLD_SCALE = 25.0    # reference gym_kilobots/lib/body.py:7


class KbConfig(C.Structure):
    _fields_ = [
        ('num_envs', C.c_int32), ('num_bots', C.c_int32), ('num_objects', C.c_int32),
        ('world_width', C.c_float), ('world_height', C.c_float),
        ('dt', C.c_float), ('vel_iters', C.c_int32), ('pos_iters', C.c_int32),
        ('drive_mode', C.c_int32), ('light_type', C.c_int32),
        ('bot_radius', C.c_float), ('bot_density', C.c_float),
        ('bot_linear_damping', C.c_float), ('bot_angular_damping', C.c_float),
        ('light_radius', C.c_float),
        ('light_lo', C.c_float * 2), ('light_hi', C.c_float * 2),
        ('light_act_lo', C.c_float * 2), ('light_act_hi', C.c_float * 2),
        ('light_max_velocity', C.c_float),
        ('ws_slots', C.c_int32),
        ('obj_radius', C.c_float * MAX_OBJECTS),
        ('obj_density', C.c_float), ('obj_friction', C.c_float),
        ('obj_linear_damping', C.c_float), ('obj_angular_damping', C.c_float),
        ('toi_walls', C.c_int32),
        ('solver_mode', C.c_int32),
        ('light_count', C.c_int32), ('light_kind', C.c_int32 * MAX_LIGHTS),
        ('lightc_radius', C.c_float * MAX_LIGHTS), ('lightc_max_velocity', C.c_float * MAX_LIGHTS),
        ('lightc_lo', (C.c_float * 2) * MAX_LIGHTS), ('lightc_hi', (C.c_float * 2) * MAX_LIGHTS),
        ('lightc_act_lo', (C.c_float * 2) * MAX_LIGHTS), ('lightc_act_hi', (C.c_float * 2) * MAX_LIGHTS),
        ('obj_shape', C.c_int32 * MAX_OBJECTS), ('obj_nverts', C.c_int32 * MAX_OBJECTS),
        ('obj_verts', ((C.c_float * 2) * MAX_POLY_VERTS) * MAX_OBJECTS),
        ('wall_friction', C.c_float),
        ('num_fixtures', C.c_int32), ('obj_fixture_body', C.c_int32 * MAX_OBJECTS),
        ('damping_model', C.c_int32), ('sense_radius', C.c_float), ('contact_capacity', C.c_int32),
        ('mode_density', C.c_float * 5),
        ('allow_sleep', C.c_int32),
    ]


class KbOutline(C.Structure):
    """kb_outline: the geometry kb_sense_objects reads, fixtures grouped by body in stable order (kb_get_outline)."""
    _fields_ = [('num_objects', C.c_int32), ('num_fixtures', C.c_int32), ('arena', C.c_float * 4),
                ('body', C.c_int32 * MAX_OBJECTS), ('kind', C.c_int32 * MAX_OBJECTS), ('nverts', C.c_int32 * MAX_OBJECTS),
                ('radius', C.c_float * MAX_OBJECTS), ('verts', ((C.c_float * 2) * MAX_POLY_VERTS) * MAX_OBJECTS)]


class KbRenderStyle(C.Structure):
    """kb_render_style: the colours of kb_render as (R, G, B) bytes; kb_render_default_style fills in the reference's."""
    _fields_ = [('table', C.c_uint8 * 3), ('body', C.c_uint8 * 3), ('ring', C.c_uint8 * 3), ('mark', C.c_uint8 * 3), ('light', C.c_uint8 * 3),
                ('light_alpha', C.c_uint8), ('obj', (C.c_uint8 * 3) * MAX_OBJECTS)]


class KbResetParams(C.Structure):
    _fields_ = [('seed', C.c_uint64), ('env_offset', C.c_int32), ('mean', C.c_float * 2), ('std', C.c_float),
                ('random_theta', C.c_int32), ('random_velocity', C.c_int32), ('resolve', C.c_int32)]


_P = C.c_void_p


class KbEpisodeInit(C.Structure):
    """kb_episode_init: what kb_reset_envs puts the selected envs at besides the spawn; device pointers, every one optional."""
    _fields_ = [('d_episode', _P), ('d_obj_pose', _P), ('d_light_pos', _P), ('d_light_vel', _P)]

BUFFER_FIELDS = ['x', 'y', 'theta', 'v', 'w', 'acc_v', 'acc_w', 'motor_l', 'motor_r',
                 'pt_threshold', 'pt_update', 'pt_nochange', 'pt_dir',
                 'light_x', 'light_y', 'light_vx', 'light_vy',
                 'ox', 'oy', 'otheta', 'ovx', 'ovy', 'ow',
                 'ws_key', 'ws_acc', 'ws_cnt',
                 'light_value', 'light_gx', 'light_gy', 'cmd_vx', 'cmd_vy', 'cmd_w', 'status', 'scratch', 'ows_acc', 'nbr_count',
                 'sleep_time', 'osleep', 'bot_mode']


class KbBuffers(C.Structure):
    _fields_ = [(n, _P) for n in BUFFER_FIELDS]


_I, _F = C.c_int, C.c_float
# every function include/kilobots_hip.h declares as (restype, argtypes): the one statement of the C ABI on this side, which
# tests/test_abi_cpu.py holds against the header's prototypes
SIGNATURES = {
    'kb_create': (_I, [C.POINTER(KbConfig), _P]),
    'kb_destroy': (None, [_P]),
    'kb_bind': (_I, [_P, C.POINTER(KbBuffers)]),
    'kb_set_actions': (_I, [_P, _P, _P]),
    'kb_step': (_I, [_P, _P, _P, _I, _I, _P]),
    'kb_get_poses': (_I, [_P, _P, _P]),
    'kb_get_state': (_I, [_P, _P, _P]),
    'kb_sense': (_I, [_P, _F, _P, _P]),
    'kb_sense_neighbors': (_I, [_P, _F, _I, _P, _P, _P, _P]),
    'kb_sense_edges': (_I, [_P, _F, _P, C.c_int64, _P, _P, _P, _P, _P]),
    'kb_sense_histogram': (_I, [_P, _F, _I, _I, _P, _P, _P]),
    'kb_histogram_sectors': (_I, [_I, _P]),
    'kb_sense_reduce': (_I, [_P, _F, _I, _I, _F, _P, _P, _P, _P]),
    'kb_sense_hops': (_I, [_P, _F, _P, _I, _P, _P, _P, _P, _P]),
    'kb_sense_clusters': (_I, [_P, _F, _P, _P, _P, _P, _P, _P]),
    'kb_get_outline': (_I, [_P, C.POINTER(KbOutline)]),
    'kb_sense_objects': (_I, [_P, _P, _P, _P]),
    'kb_grid_channels': (_I, [_P, _I]),
    'kb_sense_grid': (_I, [_P, _I, _I, _I, _P, _P]),
    'kb_sense_coverage': (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _P]),
    'kb_field_step': (_I, [_P, _I, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P]),
    'kb_path_costs': (_I, [_P, _I, _I, _P]),
    'kb_sense_paths': (_I, [_P, _I, _I, _P, _P, _I, _F, _P, _P, _P, _P, _P]),
    'kb_sense_targets': (_I, [_P, _P, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P, _P]),
    'kb_sense_assign': (_I, [_P, _P, _I, _I, _F, _F, _P, _P, _P, _P, _P, _P, _P, _P]),
    'kb_sense_contacts': (_I, [_P, _I, _F, _P, _P, _P, _P, _P]),
    'kb_render_default_style': (_I, [C.POINTER(KbRenderStyle)]),
    'kb_render': (_I, [_P, _I, _I, _I, C.POINTER(KbRenderStyle), _P, _P, _P, _P]),
    'kb_ray_directions': (_I, [_I, _P]),
    'kb_sense_rays': (_I, [_P, _F, _I, _I, _P, _P, _P]),
    'kb_light_sense': (_I, [_P, _P, _P]),
    'kb_reset': (_I, [_P, C.POINTER(KbResetParams), _P]),
    'kb_step_envs': (_I, [_P, _P, _P, _P, _I, _I, _P]),
    'kb_reset_envs': (_I, [_P, C.POINTER(KbResetParams), _P, C.POINTER(KbEpisodeInit), _P]),
    'kb_lds_bytes': (_I, [_P]),
    'kb_resident_envs_per_cu': (_I, [_P]),
    'kb_contact_capacity': (_I, [_P]),
    'kb_lds_staging_entries': (_I, [_P]),
    'kb_scratch_bytes': (C.c_size_t, [_P]),
    'kb_light_action_dim': (_I, [_P]),
    'kb_light_count': (_I, [_P]),
    'kb_block_threads': (_I, [_P]),
    'kb_variant_index': (_I, [_P]),
    'kb_set_block_threads': (_I, [_P, _I]),
    'kb_exact_division': (_I, [_P]),
    'kb_exact_selftest': (_I, [_P, _P, _P]),
    'kb_debug_lds': (_I, [_I, C.c_uint32, _P, _P]),
    'kb_last_error': (C.c_char_p, []),
    'kb_version': (C.c_char_p, []),
}
EXPORTS = list(SIGNATURES)
# an older build of the library that KB_HIP_LIB selects for an A/B (tools/ab_bench.py) has not got these: it loads, and calling
# one of them on it raises AttributeError
OPTIONAL = {'kb_step_envs', 'kb_reset_envs', 'kb_debug_lds', 'kb_sense_clusters', 'kb_sense_paths', 'kb_sense_assign'}

_lib = None


class KilobotsHipError(RuntimeError):
    pass


STATUS_BITS = {
    1: 'contact capacity overflow: contacts were dropped (raise kb_config.contact_capacity or spread the spawn)',
    2: 'warm-start slot overflow: a kilobot touches more partners than kb_config.ws_slots, their impulses are not carried over',
    4: 'a device staging limit was exceeded (more than 64 kilobots on one fixture, a rank above 255 in one (cell, direction) group of contacts, more than 63 partners of one kilobot in one direction, or a contact dependency chain deeper than the level table of the cooperative sweep: 44 x waves - 2 levels)',
    8: 'continuous step skipped for some kilobots: more kilobots that may meet a wall in one substep than the kernel keeps candidates for (min(kb_lds_staging_entries, num_bots); half the staging entries with objects or mixed drive laws)',
}


class KilobotsStatusError(KilobotsHipError):
    """A capacity limit of the device step was hit: the trajectories of the flagged envs are degraded."""


def describe_status(bits):
    return '; '.join(msg for b, msg in sorted(STATUS_BITS.items()) if bits & b) or 'ok'


def report_status(mode, where, bits, envs=''):
    """The end of every status check that found `bits` set: KilobotsStatusError for mode 'raise', otherwise a RuntimeWarning
    charged to whoever called the method that checked.  envs: what the message says of how many envs are flagged."""
    msg = '%sdevice step status 0x%x%s: %s' % (where and where + ': ', bits, envs, describe_status(bits))
    if mode == 'raise':
        raise KilobotsStatusError(msg)
    import warnings
    warnings.warn(msg, RuntimeWarning, stacklevel=4)


def load():
    """dlopen the HIP library; fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KilobotsHipError(
            'libkilobots_hip.so is missing (%s). Build it with `python -m gym_kilobots_amd.build` '
            '(needs hipcc; cross-compiles for gfx950 without a GPU). There is no CPU fallback.' % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    own = LIB_PATH == os.path.join(HERE, 'libkilobots_hip.so')
    for name, (restype, argtypes) in SIGNATURES.items():
        if own or name not in OPTIONAL or hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def check(rc, what):
    if rc != KB_OK:
        msg = load().kb_last_error().decode('utf-8', 'replace')
        raise KilobotsHipError('%s failed (%d): %s' % (what, rc, msg))


def call(lib, name, *args):
    """lib.name(*args), checked under the entry's own name."""
    check(getattr(lib, name)(*args), name)


def capturing():
    """Whether the current stream is being captured into a graph (torch.cuda.graph); False where there is no device."""
    import torch
    try:
        return bool(torch.cuda.is_current_stream_capturing())
    except (RuntimeError, AssertionError):      # (no device, or torch built without one: nothing can be capturing)
        return False


def refuse_capture(what, instead):
    """ValueError if the current stream is being captured into a graph: `what` has to read the device, which a capture cannot
    hold -- the runtime would invalidate the whole capture with an error that names nothing.  instead: what the caller can
    do.  Called before the first launch of the path, so that the capture stays valid and can go on."""
    if capturing():
        raise ValueError('%s reads the device back and cannot be captured in a graph: %s' % (what, instead))


def check_radius(radius_m, name='radius_m'):
    """A radius in metres as a float; ValueError unless it is positive."""
    radius_m = float(radius_m)
    if not radius_m > 0.0:
        raise ValueError('%s must be positive' % name)
    return radius_m


def _mask(value, bits, what, prefix):
    """An integer mask, a name or an iterable of names (the keys of `bits`) as a validated mask.  what: the argument's name,
    prefix: that of the constants, for the messages."""
    if isinstance(value, str):
        value = (value,)
    if not isinstance(value, int):
        mask = 0
        for name in value:
            if name not in bits:
                raise ValueError('%s must be a %s_* mask or made of %s and %r' % (what, prefix, ', '.join(map(repr, list(bits)[:-1])), list(bits)[-1]))
            mask |= bits[name]
        value = mask
    if isinstance(value, bool) or value <= 0 or value & ~sum(bits.values()):
        raise ValueError('%s must be a non-empty subset of %s' % (what, ' | '.join('%s_%s' % (prefix, name.upper()) for name in bits)))
    return value


def check_histogram_grid(n_rings, n_sectors):
    """The limits of kb_sense_histogram on the bin grid; ValueError where the library would answer KB_EINVAL."""
    n_rings, n_sectors = int(n_rings), int(n_sectors)
    if not 1 <= n_rings <= HIST_MAX_RINGS:
        raise ValueError('n_rings must be in 1..%d' % HIST_MAX_RINGS)
    if n_sectors != 1 and (n_sectors < 2 or n_sectors > HIST_MAX_SECTORS or n_sectors % 2):
        raise ValueError('n_sectors must be 1 or an even number in 2..%d' % HIST_MAX_SECTORS)
    if n_rings * n_sectors > HIST_MAX_BINS:
        raise ValueError('n_rings * n_sectors must not exceed %d' % HIST_MAX_BINS)
    return n_rings, n_sectors


REDUCE_OPS = {'sum': REDUCE_SUM, 'min': REDUCE_MIN, 'max': REDUCE_MAX}


def check_reduce(op, n_channels, scale):
    """The limits of kb_sense_reduce on op ('sum' | 'min' | 'max' or REDUCE_*), channel count and scale (the sum's only);
    ValueError where the library would answer KB_EINVAL.  Returns (op as an integer, n_channels, scale)."""
    if isinstance(op, str):
        if op not in REDUCE_OPS:
            raise ValueError("op must be 'sum', 'min' or 'max'")
        op = REDUCE_OPS[op]
    op, n_channels, scale = int(op), int(n_channels), float(scale)
    if op not in (REDUCE_SUM, REDUCE_MIN, REDUCE_MAX):
        raise ValueError('op must be REDUCE_SUM, REDUCE_MIN or REDUCE_MAX')
    if not 1 <= n_channels <= REDUCE_MAX_CHANNELS:
        raise ValueError('n_channels must be in 1..%d' % REDUCE_MAX_CHANNELS)
    if op == REDUCE_SUM and not 0.0 < scale < float('inf'):
        raise ValueError('scale must be finite and positive')
    return op, n_channels, scale


GRID_PLANES = {'count': GRID_COUNT, 'flow': GRID_FLOW, 'objects': GRID_OBJECTS}


def check_grid(width, height, planes):
    """The limits of kb_sense_grid on the grid and the planes (a GRID_* mask or an iterable of 'count' | 'flow' | 'objects');
    ValueError where the library would answer KB_EINVAL -- but for 'objects' on a handle without objects, which only the
    handle knows.  Returns (width, height, planes as an integer mask)."""
    width, height = int(width), int(height)
    if not (1 <= width <= GRID_MAX_SIDE and 1 <= height <= GRID_MAX_SIDE):
        raise ValueError('width and height must be in 1..%d' % GRID_MAX_SIDE)
    return width, height, _mask(planes, GRID_PLANES, 'planes', 'GRID')


def check_coverage(width, height):
    """The limits of kb_sense_coverage on the grid; ValueError where the library would answer KB_EINVAL.  Returns (width,
    height)."""
    if isinstance(width, bool) or isinstance(height, bool):
        raise ValueError('width and height must be integers')
    width, height = int(width), int(height)
    if not (1 <= width <= GRID_MAX_SIDE and 1 <= height <= GRID_MAX_SIDE):
        raise ValueError('width and height must be in 1..%d' % GRID_MAX_SIDE)
    return width, height


def check_field(width, height, channels, keep, spread, iters):
    """The limits of kb_field_step on the grid, the channel count, keep and spread (a number for all channels or one per
    channel) and the iterations; ValueError where the library would answer KB_EINVAL.  Returns (width, height, channels, keep
    and spread as tuples of `channels` floats, iters)."""
    if any(isinstance(v, bool) for v in (width, height, channels, iters)):
        raise ValueError('width, height, channels and iters must be integers')
    width, height, channels, iters = int(width), int(height), int(channels), int(iters)
    if not (1 <= width <= GRID_MAX_SIDE and 1 <= height <= GRID_MAX_SIDE):
        raise ValueError('width and height must be in 1..%d' % GRID_MAX_SIDE)
    if not 1 <= channels <= FIELD_MAX_CHANNELS:
        raise ValueError('channels must be in 1..%d' % FIELD_MAX_CHANNELS)

    def per_channel(v, name, hi):
        v = tuple(_f32(float(c)) for c in v) if hasattr(v, '__len__') else (_f32(float(v)),) * channels
        if len(v) != channels or not all(0.0 <= c <= hi for c in v):
            raise ValueError('%s must be a number or %d numbers in [0, %g]' % (name, channels, hi))
        return v
    keep, spread = per_channel(keep, 'keep', 1.0), per_channel(spread, 'spread', 0.25)
    if not 0 <= iters <= FIELD_MAX_ITERS:
        raise ValueError('iters must be in 0..%d' % FIELD_MAX_ITERS)
    return width, height, channels, keep, spread, iters


def check_paths(width, height, clearance_m=0.0):
    """The limits of kb_sense_paths on the grid and the clearance; ValueError where the library would answer KB_EINVAL.
    Returns (width, height, clearance_m)."""
    width, height = check_coverage(width, height)
    clearance_m = float(clearance_m)
    if not 0.0 <= clearance_m < float('inf'):
        raise ValueError('clearance_m must be finite and not negative')
    return width, height, clearance_m


def check_path_objects(objects, num_objects):
    """The objects that block the paths of kb_sense_paths as a mask: 'all', a mask below 2^num_objects or an iterable of object
    indices; ValueError where the library would answer KB_EINVAL."""
    if isinstance(objects, str):
        if objects != 'all':
            raise ValueError("objects must be 'all', a mask or an iterable of object indices")
        return (1 << num_objects) - 1
    if isinstance(objects, bool):
        raise ValueError("objects must be 'all', a mask or an iterable of object indices")
    if not isinstance(objects, int):
        mask = 0
        for m in objects:
            if isinstance(m, bool) or not 0 <= int(m) < num_objects:
                raise ValueError('objects: object indices must be in 0..%d' % (num_objects - 1))
            mask |= 1 << int(m)
        objects = mask
    if not 0 <= objects < (1 << num_objects):
        raise ValueError('objects must be a mask below 2^num_objects (%d objects)' % num_objects)
    return objects


def path_cells(arena, points_m, width, height):
    """The uint8 mask [E, height, width] ([1, height, width] for shared points) of the cells of kb_sense_grid's width x height
    grid over arena = (xmin, xmax, ymin, ymax) in world units (kb_outline.arena) that points in metres fall in: points_m
    array-like [E, K, 2] or [K, 2].  The cell rule of the header in float32, every operation rounded on its own: world
    units = metres * 25.0f;  t = (v - min) * ((float)n / (max - min));  cell 0 if !(t > 0) (NaN included), n - 1 if t >= n,
    otherwise the truncation of t.  Host only."""
    import numpy as np
    width, height = check_coverage(width, height)
    f32 = np.float32
    pts = np.asarray(points_m, dtype=f32)
    if pts.ndim not in (2, 3) or pts.shape[-1] != 2:
        raise ValueError('points_m must have the shape (K, 2) or (E, K, 2)')
    pts = pts.reshape((-1,) + pts.shape[-2:])
    xmin, xmax, ymin, ymax = (f32(v) for v in arena)

    def axis(v, lo, hi, n):
        with np.errstate(invalid='ignore', over='ignore'):
            t = (v * f32(WORLD_SCALE) - lo) * (f32(n) / (hi - lo))
            low, high = ~(t > 0), t >= f32(n)
            return np.where(low, 0, np.where(high, n - 1, np.where(low | high, f32(0), t).astype(np.int64)))
    ix, iy = axis(pts[..., 0], xmin, xmax, width), axis(pts[..., 1], ymin, ymax, height)
    mask = np.zeros((pts.shape[0], height * width), dtype=np.uint8)
    np.put_along_axis(mask, iy * width + ix, 1, axis=1)
    return mask.reshape(-1, height, width)


def check_targets(n_targets, tol_m):
    """The limits of kb_sense_targets on the number of slots and the tolerance in metres; ValueError where the library would
    answer KB_EINVAL.  Returns (n_targets, tol_m)."""
    if isinstance(n_targets, bool) or isinstance(tol_m, bool):
        raise ValueError('n_targets must be an integer and tol_m a number')
    n_targets, tol_m = int(n_targets), float(tol_m)
    if not 1 <= n_targets <= MAX_TARGETS:
        raise ValueError('n_targets must be in 1..%d' % MAX_TARGETS)
    if not 0.0 <= tol_m < float('inf'):
        raise ValueError('tol_m must be finite and not negative')
    return n_targets, tol_m


def check_assign(n_targets, tol_m, cutoff_m):
    """The limits of kb_sense_assign: those of kb_sense_targets, and a cutoff in metres that is a number and not negative
    (None and +inf: no cutoff); ValueError where the library would answer KB_EINVAL.  Returns (n_targets, tol_m, cutoff_m)."""
    n_targets, tol_m = check_targets(n_targets, tol_m)
    if isinstance(cutoff_m, bool):
        raise ValueError('cutoff_m must be a number or None')
    cutoff_m = float('inf') if cutoff_m is None else float(cutoff_m)
    if not cutoff_m >= 0.0:
        raise ValueError('cutoff_m must not be negative (None or inf: no cutoff)')
    return n_targets, tol_m, cutoff_m


RENDER_LAYERS = {'objects': RENDER_OBJECTS, 'bots': RENDER_BOTS, 'light': RENDER_LIGHT}
RENDER_STYLE_FIELDS = ('table', 'body', 'ring', 'mark', 'light', 'light_alpha', 'obj')


def check_render(width, height, layers):
    """The limits of kb_render on the frame and the layers (a RENDER_* mask or an iterable of 'objects' | 'bots' | 'light');
    ValueError where the library would answer KB_EINVAL.  Returns (width, height, layers as an integer mask)."""
    width, height = int(width), int(height)
    if not (1 <= width <= RENDER_MAX_SIDE and 1 <= height <= RENDER_MAX_SIDE):
        raise ValueError('width and height must be in 1..%d' % RENDER_MAX_SIDE)
    return width, height, _mask(layers, RENDER_LAYERS, 'layers', 'RENDER')


def render_style(style=None):
    """A KbRenderStyle: the defaults (kb_render_default_style) with the keys of the dict `style` written over them.  Colours
    are (R, G, B) in 0..255, 'light_alpha' one such number, 'obj' a list of up to MAX_OBJECTS colours (the rest keep the
    default).  ValueError for an unknown key or a value outside a byte."""
    st = KbRenderStyle()
    call(load(), 'kb_render_default_style', C.byref(st))

    def colour(dst, v, key):
        v = [int(c) for c in v]
        if len(v) != 3 or not all(0 <= c <= 255 for c in v):
            raise ValueError('style[%r] must be (R, G, B) in 0..255' % key)
        for i in range(3):
            dst[i] = v[i]
    for key, v in dict(style or {}).items():
        if key not in RENDER_STYLE_FIELDS:
            raise ValueError('style: unknown key %r (the keys are %s)' % (key, ', '.join(RENDER_STYLE_FIELDS)))
        if key == 'light_alpha':
            if not 0 <= int(v) <= 255:
                raise ValueError("style['light_alpha'] must be in 0..255")
            st.light_alpha = int(v)
        elif key == 'obj':
            v = list(v)
            if len(v) > MAX_OBJECTS:
                raise ValueError("style['obj'] holds at most %d colours" % MAX_OBJECTS)
            for m, c in enumerate(v):
                colour(st.obj[m], c, 'obj')
        else:
            colour(getattr(st, key), v, key)
    return st


RAY_TARGETS = {'bots': RAY_BOTS, 'objects': RAY_OBJECTS, 'walls': RAY_WALLS}


def check_rays(radius_m, n_rays, targets):
    """The limits of kb_sense_rays on the radius, the ray count and the targets (a RAY_* mask or an iterable of 'bots' |
    'objects' | 'walls'); ValueError where the library would answer KB_EINVAL -- but for 'objects' on a handle without
    objects, which only the handle knows.  Returns (radius_m, n_rays, targets as an integer mask)."""
    radius_m, n_rays = check_radius(radius_m), int(n_rays)
    if not 1 <= n_rays <= MAX_RAYS:
        raise ValueError('n_rays must be in 1..%d' % MAX_RAYS)
    return radius_m, n_rays, _mask(targets, RAY_TARGETS, 'targets', 'RAY')


def ray_directions(n_rays):
    """The directions u_k, k = 0 .. n_rays - 1, that kb_sense_rays hands its kernel (kb_ray_directions): a list of (x, y)
    floats in the kilobot's frame, ray 0 dead ahead, counter-clockwise; no handle and no device needed."""
    n = int(n_rays)
    buf = (C.c_float * (2 * max(min(n, MAX_RAYS), 1)))()
    call(load(), 'kb_ray_directions', n, buf)
    return [(buf[2 * k], buf[2 * k + 1]) for k in range(n)]


def check_edges(radius_m, capacity=None):
    """The limits of kb_sense_edges on the radius and the capacity (None: the caller sizes the outputs from the counts);
    ValueError where the library would answer KB_EINVAL.  Returns (radius_m, capacity)."""
    radius_m = check_radius(radius_m)
    if capacity is not None:
        if isinstance(capacity, bool) or int(capacity) != capacity:
            raise ValueError('capacity must be an integer or None')
        capacity = int(capacity)
        if capacity < 0:
            raise ValueError('capacity must not be negative')
    return radius_m, capacity


def _f32(v):
    return C.c_float(v).value


def render_bands(num_bots, world_width, world_height, bot_radius, width, height):
    """(bands, rows per band) of kb_render for a handle of this shape and a frame of this size: the host rule of RenderLds
    (csrc/kb_sense.h) restated, with the broadphase grid of kb_create.  A band's bytes are staged in what the
    64 KiB of dynamic LDS leave behind the cell lists (3 width bytes per row, 32 kept back for alignment), a band holds at
    most 8192 pixels and at least one row; the fewest such bands, rows spread evenly."""
    cell = 0.875
    while cell < _f32(_f32(2.0 * _f32(bot_radius)) * 25.0):
        cell *= 2.0
    W, H = _f32(_f32(world_width) * 25.0), _f32(_f32(world_height) * 25.0)
    while True:
        inv = _f32(1.0 / cell)
        gw, gh = max(1, int(-(-_f32(W * inv) // 1))), max(1, int(-(-_f32(H * inv) // 1)))
        if gw * gh <= 8192:
            break
        cell *= 2.0
    NP = (int(num_bots) + 3) & ~3
    objects_image = 16 * MAX_OBJECTS + 32 * MAX_OBJECTS * MAX_POLY_VERTS + 8 * MAX_OBJECTS + 16 * ((MAX_OBJECTS + 4) // 4)
    stage = (objects_image + 4 * MAX_OBJECTS + 16 * MAX_LIGHTS + 16 + 20 * NP + 2 * ((gw * gh + 1) & ~1) + 15) & ~15
    room = 64 * 1024 - stage
    max_rows = max(1, min((room - 32) // (3 * width), 8192 // width))
    bands = (height + max_rows - 1) // max_rows
    return bands, (height + bands - 1) // bands


def histogram_sectors(n_sectors):
    """The sector boundaries u_m, m = 1 .. n_sectors / 2 - 1, that kb_sense_histogram hands its kernel
    (kb_histogram_sectors): a list of (x, y) floats; no handle and no device needed."""
    n = int(n_sectors)
    rows = max(n // 2 - 1, 0)
    buf = (C.c_float * (2 * max(rows, 1)))()
    call(load(), 'kb_histogram_sectors', n, buf)
    return [(buf[2 * m], buf[2 * m + 1]) for m in range(rows)]


def outline(handle):
    """The geometry kb_sense_objects reads for a handle (kb_get_outline) as a KbOutline: the arena bounds and the fixtures
    grouped by body in stable order, world units; no device and no bound buffers needed."""
    o = KbOutline()
    call(load(), 'kb_get_outline', handle, C.byref(o))
    return o


def default_config(num_envs, num_bots, drive_mode=DRIVE_VELOCITY, light_type=LIGHT_NONE, **kw):
    """Reference defaults: kilobots_env.py:19,25-28; kilobot.py:9,25-30,214; body.py:11-16; light.py:49-54,152."""
    inf = float('inf')
    c = KbConfig()
    c.num_envs, c.num_bots, c.num_objects = num_envs, num_bots, 0
    for i in range(MAX_OBJECTS):
        c.obj_radius[i] = 0.075
    c.world_width, c.world_height = 2.0, 1.5
    c.dt, c.vel_iters, c.pos_iters = 0.1, 10, 10
    c.drive_mode, c.light_type = drive_mode, light_type
    c.bot_radius = 0.0165
    c.bot_density = 2.0 if drive_mode in (DRIVE_VELOCITY, DRIVE_ACCEL) else 1.0
    c.bot_linear_damping = c.bot_angular_damping = 0.8
    c.light_radius = 0.2
    c.light_lo[0] = c.light_lo[1] = -inf
    c.light_hi[0] = c.light_hi[1] = inf
    c.light_act_lo[0] = c.light_act_lo[1] = -0.01
    c.light_act_hi[0] = c.light_act_hi[1] = 0.01
    c.light_max_velocity = inf
    c.ws_slots = 32     # contacts per kilobot whose impulse is carried over (Box2D keeps every b2Contact; 32 covers a dense overlapping spawn)
    c.obj_density, c.obj_friction = 2.0, 0.01
    c.obj_linear_damping = c.obj_angular_damping = 0.8
    c.toi_walls = 1      # b2World continuousPhysics defaults to true
    c.wall_friction = 0.2  # b2FixtureDef default (the arena chain, kilobots_env.py:46-51)
    c.solver_mode = 0
    c.damping_model = DAMPING_PADE
    c.sense_radius = 0.0
    c.contact_capacity = 0
    c.allow_sleep = 1      # b2World(gravity=(0, 0), doSleep=True) of kilobots_env.py:45; 0 drops the sleep state
    c.light_count = 1
    for i in range(MAX_LIGHTS):
        c.light_kind[i] = LIGHT_CIRCULAR
        c.lightc_radius[i] = 0.2
        c.lightc_max_velocity[i] = inf
        for k in range(2):
            c.lightc_lo[i][k], c.lightc_hi[i][k] = -inf, inf
            c.lightc_act_lo[i][k], c.lightc_act_hi[i][k] = -0.01, 0.01
    for k, v in kw.items():
        _assign(c, k, v)
    return c


def _assign(c, k, v):
    cur = getattr(c, k)
    if hasattr(cur, '__len__'):
        _fill(cur, v)
    else:
        setattr(c, k, v)


def _fill(dst, src):
    for i, vi in enumerate(src):
        if hasattr(dst[i], '__len__'):
            _fill(dst[i], vi)
        else:
            dst[i] = vi
