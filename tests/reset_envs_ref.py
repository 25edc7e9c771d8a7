"""References for kb_step_envs / kb_reset_envs (masked stepping and per-env reset), on the CPU oracle:

  spawn()            the draw of kbo_reset restated in numpy for any word z of the Philox counter (z = 0 is kbo_reset itself),
                     through the oracle's own kbo_philox4x32_10, kbo_logf and kbo_sincosf;
  masked()           run something on every env of an OracleSim and put the unselected envs back: envs do not interact, so
                     this IS a masked step / a masked reset;
  ref_reset_envs()   kb_reset_envs as the header states it, from the two above;
  MaskedOracleBackend  the oracle backend of tests/oracle_backend.py with step(env_mask=) and reset_envs(), so that
                     BatchedKilobotsEnv runs its per-env episodes on the CPU;
  CASES, masks(), ... the shapes and scenes that the CPU file checks for vacuity and the GPU file runs on the device."""
import ctypes as C

import numpy as np
import torch

from oracle import oracle as O
from tests import scenes
from tests.oracle_backend import OracleBackend

STATE_FIELDS = [n for n, _ in O.State._fields_]
f32 = np.float32


# ---------------------------------------------------------------------------------------------- masked()
def snapshot(osim):
    return {n: getattr(osim, n).copy() for n in STATE_FIELDS}


def restore(osim, snap, rows=None):
    """Write a snapshot back IN PLACE (the oracle holds pointers to the arrays): every env, or the envs `rows` selects."""
    for n, a in snap.items():
        cur = getattr(osim, n)
        if rows is None:
            cur[...] = a
        else:
            cur[rows] = a[rows]


def masked(osim, mask, fn):
    """fn() acts on all envs of osim; afterwards every state array of the envs with mask == 0 is what it was."""
    mask = np.asarray(mask).astype(bool)
    snap = snapshot(osim)
    fn()
    restore(osim, snap, ~mask)


# ---------------------------------------------------------------------------------------------- the spawn, restated
def spawn(cfg, seed=0, z=0, env_offset=0, mean=(0.0, 0.0), std=0.1, random_theta=False, random_velocity=False):
    """(x, y, theta, v, w), each [E, N] float32: what kbo_reset (kb_oracle.c) writes for the Philox counter
    (env_offset + e, b, z[e], 0); every operation one fp32 operation, in its order.  v, w: the command of a velocity or
    acceleration kilobot (the other laws do not store one)."""
    L = O.lib()
    E, N = cfg.num_envs, cfg.num_bots
    z = np.broadcast_to(np.asarray(z, np.int64), (E,))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = (C.c_uint32 * 2)(seed & 0xFFFFFFFF, seed >> 32)
    W, H = f32(cfg.world_width), f32(cfg.world_height)
    lo_x, hi_x = f32(-0.5) * W + f32(0.02), f32(0.5) * W - f32(0.02)
    lo_y, hi_y = f32(-0.5) * H + f32(0.02), f32(0.5) * H - f32(0.02)
    m0, m1, sd = f32(mean[0]), f32(mean[1]), f32(std)
    inv24, inv16 = f32(1.0) / f32(16777216.0), f32(1.0) / f32(65536.0)
    two_pi, pi, scale = f32(6.28318530717958647692), f32(3.14159265358979323846), f32(O.WORLD_SCALE)
    half_pi = f32(0.5) * pi
    ctr, r = (C.c_uint32 * 4)(), (C.c_uint32 * 4)()
    sn, cs = C.c_float(), C.c_float()
    x, y, th, v, w = (np.zeros((E, N), np.float32) for _ in range(5))
    for e in range(E):
        for b in range(N):
            ctr[0], ctr[1], ctr[2], ctr[3] = (env_offset + e) & 0xFFFFFFFF, b, int(z[e]) & 0xFFFFFFFF, 0
            L.kbo_philox4x32_10(ctr, key, r)
            u1 = f32((r[0] >> 8) + 1) * inv24
            u2 = f32(r[1] >> 8) * inv24
            rad = np.sqrt(f32(-2.0) * f32(L.kbo_logf(float(u1))))
            L.kbo_sincosf(float(two_pi * u2), C.byref(sn), C.byref(cs))
            xm = m0 + sd * (rad * f32(cs.value))
            ym = m1 + sd * (rad * f32(sn.value))
            xm = np.minimum(np.maximum(xm, lo_x), hi_x)
            ym = np.minimum(np.maximum(ym, lo_y), hi_y)
            x[e, b], y[e, b] = xm * scale, ym * scale
            if random_theta:
                th[e, b] = (f32(r[2] >> 8) * inv24 * f32(2.0) - f32(1.0)) * pi
            if random_velocity:
                v[e, b] = f32(r[3] & 0xFFFF) * inv16 * f32(0.01)
                w[e, b] = (f32(r[3] >> 16) * inv16 * f32(2.0) - f32(1.0)) * half_pi
    return x, y, th, v, w


# ---------------------------------------------------------------------------------------------- kb_reset_envs
def ref_reset_envs(osim, mask, seed=0, mean=(0.0, 0.0), std=0.1, random_theta=False, random_velocity=False, resolve=True, env_offset=0,
                   episode=None, objects=None, lights=None, light_vel=None, draw=None):
    """kb_reset_envs on an OracleSim.  episode: [E] counter words (None: 0, kbo_reset as it is); objects [E, M, 3] world units;
    lights / light_vel [E, L, 2] (or [E, 2]).  draw: spawn(...) of these very arguments, if the caller has it already."""
    cfg = osim.cfg

    def fn():
        osim.reset(seed=seed, mean=mean, std=std, random_theta=random_theta, random_velocity=random_velocity, resolve=False, env_offset=env_offset)
        if episode is not None:
            x, y, th, v, w = draw if draw is not None else spawn(cfg, seed, episode, env_offset, mean, std, random_theta, random_velocity)
            osim.x[...], osim.y[...], osim.theta[...] = x, y, th
            law = osim.bot_mode if cfg.drive_mode == O.DRIVE_MIXED else np.full(x.shape, cfg.drive_mode)
            vel = (law == O.DRIVE_VELOCITY) | (law == O.DRIVE_ACCEL)
            osim.v[vel], osim.w[vel] = v[vel], w[vel]
        if objects is not None:
            o = np.asarray(objects, np.float32)
            osim.ox[...], osim.oy[...], osim.otheta[...] = o[..., 0], o[..., 1], o[..., 2]
            for a in (osim.ovx, osim.ovy, osim.ow, osim.osleep):
                a[...] = 0.0
        if lights is not None:
            l = np.asarray(lights, np.float32)
            osim.light_x[...], osim.light_y[...] = l[..., 0].reshape(osim.light_x.shape), l[..., 1].reshape(osim.light_y.shape)
        if lights is not None or light_vel is not None:
            lv = np.zeros(osim.light_vx.shape + (2,), np.float32) if light_vel is None else np.asarray(light_vel, np.float32)
            osim.light_vx[...], osim.light_vy[...] = lv[..., 0].reshape(osim.light_vx.shape), lv[..., 1].reshape(osim.light_vy.shape)
        if resolve:
            osim.step(1, flags=O.STEP_NO_DRIVE)
    masked(osim, mask, fn)


class MaskedOracleBackend(OracleBackend):
    """OracleBackend with the two masked entry points of KilobotSim."""

    def step(self, n_substeps=1, actions=None, light_action=None, flags=0, env_mask=None):
        plain = super().step
        if env_mask is None:
            return plain(n_substeps, actions, light_action, flags)
        masked(self.o, env_mask.cpu().numpy(), lambda: plain(n_substeps, actions, light_action, flags))

    def reset_envs(self, env_mask, episode=None, objects=None, lights=None, light_vel=None, **kw):
        host = lambda t: None if t is None else t.cpu().numpy()
        ref_reset_envs(self.o, env_mask.cpu().numpy(), episode=host(episode), objects=host(objects), lights=host(lights),
                       light_vel=host(light_vel), **kw)


# ---------------------------------------------------------------------------------------------- shapes and scenes
_W = O.WORLD_SCALE
# E, N, drive law, light, std of the spawn, further configuration.  std 0.1 overlaps kilobots at every N >= 40; 1024 kilobots
# at 0.1 would overflow the default contact store (about 14 000 touching pairs), 0.3 leaves about 1 600
CASES = {
    'velocity40': dict(E=6, N=40, mode=O.DRIVE_VELOCITY, light=O.LIGHT_NONE, std=0.1, kw={}),
    'accel200': dict(E=5, N=200, mode=O.DRIVE_ACCEL, light=O.LIGHT_NONE, std=0.1, kw={}),
    'motors200': dict(E=5, N=200, mode=O.DRIVE_MOTORS, light=O.LIGHT_NONE, std=0.1, kw={}),
    'fixed1024': dict(E=3, N=1024, mode=O.DRIVE_VELOCITY, light=O.LIGHT_NONE, std=0.3, kw={}),       # the fixed-size kernel
    'objects64': dict(E=4, N=64, mode=O.DRIVE_PHOTOTAXIS, light=O.LIGHT_CIRCULAR, std=0.1,
                      kw=dict(num_objects=2, obj_shape=[O.SHAPE_CIRCLE, O.SHAPE_BOX], obj_radius=[0.06],
                              obj_verts=[[[0.0, 0.0]], [[0.075 * _W, 0.075 * _W]]])),                  # a disc and a box
    'sleep48': dict(E=4, N=48, mode=O.DRIVE_VELOCITY, light=O.LIGHT_NONE, std=0.1, kw=dict(allow_sleep=1, num_objects=1, obj_radius=[0.05])),
    'sense96': dict(E=4, N=96, mode=O.DRIVE_VELOCITY, light=O.LIGHT_NONE, std=0.1, kw=dict(sense_radius=0.07)),
}
MASK_NAMES = ('none', 'all', 'alternating', 'middle')
RESET_SEED, FIRST_SEED = 2 ** 33 + 17, 5


def masks(E):
    e = np.arange(E)
    return {'none': np.zeros(E, np.uint8), 'all': np.ones(E, np.uint8), 'alternating': (e % 2 == 0).astype(np.uint8),
            'middle': (e == E // 2).astype(np.uint8)}


def config_kw(case):
    kw = dict(CASES[case]['kw'])
    kw.setdefault('allow_sleep', 0)
    return kw


def make_oracle(case):
    c = CASES[case]
    return O.OracleSim(O.default_config(c['E'], c['N'], c['mode'], c['light'], **config_kw(case)))


def takes_actions(case):
    return CASES[case]['mode'] in (O.DRIVE_VELOCITY, O.DRIVE_ACCEL)


def actions(case, seed):
    """[E, N, 2] float32 actions of a case, None for the laws that take none"""
    c = CASES[case]
    if not takes_actions(case):
        return None
    a = scenes.random_actions(c['E'], c['N'], seed=seed).astype(np.float32)
    if c['mode'] == O.DRIVE_ACCEL:
        a = (a * 2.0 - 0.004).astype(np.float32)
    return np.ascontiguousarray(a)


def light_action(case, seed):
    c = CASES[case]
    if c['light'] == O.LIGHT_NONE:
        return None
    return np.random.RandomState(seed).uniform(-0.012, 0.012, size=(c['E'], 2)).astype(np.float32)


def first_objects_m(case):
    """where the objects lie before any masked call: [E, M, 2] metres"""
    c, M = CASES[case], CASES[case]['kw'].get('num_objects', 0)
    if M == 0:
        return None
    base = np.array([[0.4, -0.3], [-0.5, 0.35]])[:M]
    return np.tile(base[None], (c['E'], 1, 1)) + 0.01 * np.arange(c['E'])[:, None, None]


def templates(case):
    """(objects [E, M, 3] world units, lights [E, 2], light_vel [E, 2]) that the masked resets put in place; None where the case
    has no objects / no light.  Different in every env, and different from first_objects_m."""
    c, M = CASES[case], CASES[case]['kw'].get('num_objects', 0)
    E = c['E']
    e = np.arange(E, dtype=np.float64)
    objects = lights = vel = None
    if M:
        base = np.array([[0.5, 0.3, 0.2], [-0.45, -0.3, -0.4]])[:M]
        o = np.tile(base[None], (E, 1, 1))
        o[..., 0] += 0.02 * e[:, None]
        o[..., 2] += 0.1 * e[:, None]
        objects = np.ascontiguousarray(np.concatenate([(o[..., :2] * _W).astype(np.float32), o[..., 2:].astype(np.float32)], -1))
    if c['light'] != O.LIGHT_NONE:
        lights = np.ascontiguousarray(np.stack([0.1 + 0.02 * e, -0.05 - 0.01 * e], -1).astype(np.float32))
        vel = np.ascontiguousarray(np.stack([0.001 * (e + 1), -0.002 * (e + 1)], -1).astype(np.float32))
    return objects, lights, vel


def first_reset_kw(case):
    return dict(seed=FIRST_SEED, std=CASES[case]['std'], random_theta=True, random_velocity=takes_actions(case), resolve=True)


def reset_kw(case, resolve=True):
    """the kb_reset_params of the masked resets"""
    return dict(seed=RESET_SEED, mean=(0.03, -0.02), std=CASES[case]['std'], random_theta=True, random_velocity=takes_actions(case),
                resolve=resolve, env_offset=2)


def prepare(case, sims, to_device=None):
    """Every sim of `sims` (OracleSim or KilobotSim alike) from creation to the state before the masked call: objects placed,
    the full reset, mixed motor commands, then two env.steps of five substeps on every env -- so that the envs a mask leaves
    out hold contacts and are no spawn any more.  to_device: numpy -> what a KilobotSim takes (tensors on its device)."""
    c = CASES[case]
    rng = np.random.RandomState(3)
    ml = rng.randint(0, 256, size=(c['E'], c['N'])).astype(np.uint8)
    mr = rng.randint(0, 256, size=(c['E'], c['N'])).astype(np.uint8)
    for s in sims:
        oracle = isinstance(s, O.OracleSim)
        give = (lambda a: a) if oracle else to_device
        if first_objects_m(case) is not None:
            s.set_objects_m(first_objects_m(case))
        s.reset(**first_reset_kw(case))
        if c['mode'] in (O.DRIVE_MOTORS, O.DRIVE_PHOTOTAXIS):
            if oracle:
                s.motor_l[...], s.motor_r[...] = ml, mr
            else:
                s.motor_l.copy_(give(ml))
                s.motor_r.copy_(give(mr))
        for k in range(2):
            a, la = actions(case, 20 + k), light_action(case, 30 + k)
            if oracle:
                if a is not None:
                    s.set_actions(a)
                s.step(5, light_action=la)
            else:
                s.step(5, actions=None if a is None else give(a), light_action=None if la is None else give(la))
