"""What the GPU tests share: an oracle / device pair of the same scene, the bit-exact comparison of their state and of the
packed warm-start list, host <-> device copies, and small helpers of the sensing suites.  Importing this module does not
initialise the device."""
import numpy as np
import torch

from oracle import oracle as O
from tests import geometry_scenes as GS
from tests import objects_ref
from tests import reduce_ref


def make_pair(E, N, mode=O.DRIVE_VELOCITY, light=O.LIGHT_NONE, xy=None, th=None, objects=None, **kw):
    from gym_kilobots_amd.sim import KilobotSim
    if objects is not None:
        kw['num_objects'] = objects.shape[-2]
    kw.setdefault('allow_sleep', 0)      # (the library default is the reference's doSleep=True; the sleeping tests and the fuzz ask for it)
    osim = O.OracleSim(O.default_config(E, N, mode, light, **kw))
    gsim = KilobotSim(E, N, mode, light, debug_outputs=True, **kw)
    if xy is not None:
        osim.set_poses_m(xy, th)
        gsim.set_poses_m(xy, th)
    if objects is not None:
        osim.set_objects_m(objects)
        gsim.set_objects_m(objects)
    return osim, gsim


OBJ_FIELDS = ('x', 'y', 'theta', 'ox', 'oy', 'otheta', 'ovx', 'ovy', 'ow', 'ows_acc')


def cpu(t):
    return t.detach().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def put_device(sim, name, val):
    getattr(sim, name).copy_(dev(val))


def assert_same(osim, gsim, what='', fields=('x', 'y', 'theta')):
    torch.cuda.synchronize()
    for f in fields:
        a, b = getattr(osim, f), cpu(getattr(gsim, f))
        if not np.array_equal(a, b.reshape(a.shape)):
            d = np.abs(a.astype(np.float64) - b.reshape(a.shape).astype(np.float64))
            raise AssertionError('%s: field %s differs: max |d| = %.3e at %s (%d of %d elements)'
                                 % (what, f, d.max(), np.unravel_index(d.argmax(), d.shape), (d > 0).sum(), d.size))


def assert_ws_same(osim, gsim, what=''):
    torch.cuda.synchronize()
    cnt_o, cnt_g = osim.ws_cnt, cpu(gsim.ws_cnt)
    assert np.array_equal(cnt_o, cnt_g), what + ': ws_cnt differs'
    key_g, acc_g = cpu(gsim.ws_key).view(np.uint32), cpu(gsim.ws_acc)
    assert key_g.shape == osim.ws_key.shape, 'contact capacity differs between oracle and kernel'
    used = np.arange(osim.cap)[None, :] < cnt_o.astype(np.int64).sum(1)[:, None]     # packed list: first sum(cnt) entries
    assert np.array_equal(osim.ws_key[used], key_g[used]), what + ': ws_key differs'
    assert np.array_equal(osim.ws_acc[used], acc_g[used]), what + ': ws_acc differs'


def geometry_pair(g, **kw):
    """(scene, oracle sim, device sim) of a row of tests/geometry_scenes.py, both sims at the scene's start."""
    s = GS.scene(g)
    osim, gsim = make_pair(s.E, s.N, s.mode, xy=s.xy, th=s.th, **dict(s.kw, **kw))
    GS.apply_start(s, osim, GS.put_numpy)
    GS.apply_start(s, gsim, put_device)
    return s, osim, gsim


# ---- the sensing suites ----------------------------------------------------------------------------------------------------
def state(g):
    torch.cuda.synchronize()
    return cpu(g.x), cpu(g.y), cpu(g.theta)


OBJECT_STATE = ('x', 'y', 'theta', 'ox', 'oy', 'otheta')


def object_state(g):
    """The poses of kilobots and objects; None for a buffer that the sim does not have."""
    torch.cuda.synchronize()
    return [cpu(getattr(g, f)) if getattr(g, f) is not None else None for f in OBJECT_STATE]


def same_as_f32(t, w):
    """The device tensor and the array have the same bits, both taken as float32 (objects_ref.bits converts)."""
    return np.array_equal(objects_ref.bits(cpu(t)), objects_ref.bits(w))


def ranges(g, R):
    """The range matrix of every env of the sim, once per (scene, radius)."""
    x, y = state(g)[:2]
    return [reduce_ref.in_range(x[e], y[e], R) for e in range(g.num_envs)]


class Spy(object):
    """Records the calls that go through a ctypes library."""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def call(*args):
            self.calls.append((name, args))
            return fn(*args)
        return call
