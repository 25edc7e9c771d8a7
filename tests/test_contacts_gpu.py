"""kb_sense_contacts on the device against the numpy restatement (tests/contacts_ref.py) applied to the device's OWN store:
integers by equality, floats by bit pattern.  The store itself is held against the oracle's by the parity tests; S1 is
compared end to end once more here."""
import numpy as np
import pytest
import torch

from tests import contacts_ref as ref
from tests import contacts_scenes as cs
from tests import scenes
from tests.gpu_common import assert_ws_same, cpu, dev
from tests.sensing_checks import same_contacts as same, want_contacts as want
from tests.sensing_common import make_sim

pytestmark = pytest.mark.gpu

NAN = float('nan')


def run(sc, steps=None, **more):
    """The scene on the device: placed, resolved, stepped."""
    g = make_sim(sc['E'], sc['N'], **dict(sc['kw'], **more))
    cs.place(g, sc)
    g.step(1, flags=cs.STEP_NO_DRIVE)
    for _ in range(sc['steps'] if steps is None else steps):
        g.step(10, actions=dev(sc['actions']))
    return g


def check(g, ks=(8,), what=''):
    exp = None
    for k in ks:
        exp = want(g, k)
        same(g.contacts(k), exp, '%s k = %d' % (what, k))
    return exp


def test_s1_after_resolve_and_after_steps():
    sc = cs.s1()
    g = run(sc, steps=0)
    assert int(cpu(g.status).max()) == 0
    p, i, t, o = check(g, (1, 4, 8, 16, 0), 'S1 resolved')
    assert t[..., 0].max() > 16 and not t[..., 3].any() and t[..., 2].sum() > 0      # every k truncates; touching with impulse 0
    for _ in range(sc['steps']):
        g.step(10, actions=dev(sc['actions']))
    assert int(cpu(g.status).max()) == 0
    p, i, t, o = check(g, (1, 4, 8, 16, 0), 'S1 stepped')
    assert t[..., 1].sum() == 36 and t[..., 2].sum() == 9 and o[..., 0].sum() == 9 and o[..., 1].min() > 0


def test_s1_end_to_end_against_the_oracle():
    sc = cs.s1()
    _, o = cs.oracle_run(sc)
    g = run(sc)
    assert_ws_same(o, g, 'S1')
    exp = ref.contacts_ref(o.ws_cnt, o.ws_key, o.ws_acc, o.cap, sc['N'], 1, cs.fixture_body(o.cfg), 8)
    same(g.contacts(8), exp, 'S1 against the oracle')


@pytest.mark.parametrize('name', ['S2', 'S3', 'S4b'])
def test_scenes(name):
    """S2: one full tile of 256 kilobots plus a remainder; S3: four tiles, scans over 1024 owners; S4b: ws_cnt beyond 8, lists
    beyond 16 and 2000 entries per env on a store of 8192."""
    sc = cs.SCENES[name]()
    g = run(sc)
    assert int(cpu(g.status).max()) == 0
    p, i, t, o = check(g, (8, 16, 0) if name == 'S4b' else (8, 0), name)
    assert o is None and t[..., 0].sum() > 300
    if name == 'S4b':
        assert g.contact_capacity == 8192 and int(cpu(g.ws_cnt).max()) > 8 and t[..., 0].max() > 16


def test_one_kilobot_per_env_and_an_empty_store():
    g = make_sim(5, 1, np.zeros((5, 1, 2)), np.zeros((5, 1)))
    g.step(10)
    p, i, t, o = check(g, (1, 3, 0, 16), 'N = 1')
    assert (p == -1).all() and not t.any()
    sc = cs.s1()
    g = run(sc)
    assert cpu(g.contacts(8)[2]).any()
    g.forget_contacts()
    p, i, t, o = g.contacts(8)
    torch.cuda.synchronize()
    assert bool((p == -1).all()) and not cpu(i).view(np.int32).any() and not cpu(t).view(np.int32).any() and not cpu(o).view(np.int32).any()
    check(g, (8,), 'forgotten')


def test_box_scene():
    E, N = 2, 128
    xy, _ = scenes.gaussian_spawn(E, N, sigma=0.3, seed=62)
    g = make_sim(E, N, xy, scenes.toward_objects_theta(xy), num_objects=4, **scenes.shape_kw(scenes.MIXED_SHAPES))
    g.set_objects_m(np.tile(scenes.CFG4_OBJECTS[None], (E, 1, 1)), np.tile(np.array([0.3, 0.0, -0.7, 1.1])[None], (E, 1)))
    g.step(1, flags=cs.STEP_NO_DRIVE)
    a = torch.zeros(E, N, 2, device='cuda')
    a[..., 0] = 0.01
    for _ in range(4):
        g.step(10, actions=a)
    p, i, t, o = check(g, (5, 8, 0), 'boxes')
    assert o[..., 0].sum() >= 8 and (o[..., 0] > 0).sum() >= 3 and o[..., 1].max() > 0


def compound_scene():
    """Objects of scenes.compound_kw at the cfg4 positions, unrotated; kilobot 0 sits in the inner corner of the LForm (object 0,
    fixtures 0 and 3 of the config) and drives into it, kilobot 1 touches the disc (fixture 1), kilobot 2 the box (fixture 5),
    kilobots 3 and 4 each other."""
    E, N = 2, 6
    corner = np.array([-0.01875, -0.0125])      # of the LForm scaled to 0.15 x 0.15 and recentred (scenes.reference_polygon_fixtures)
    xy, th = np.zeros((E, N, 2)), np.zeros((E, N))
    xy[:, 0] = scenes.CFG4_OBJECTS[0] + corner + np.array([-0.016, 0.016])
    th[:, 0] = -np.pi / 4
    xy[:, 1] = [-0.5 - 0.065, 0.35]
    xy[:, 2] = [0.5 - 0.05 - 0.016, -0.35]
    xy[:, 3], xy[:, 4], xy[:, 5] = [0.0, 0.0], [0.02, 0.0], [-0.9, 0.0]
    xy[1] += 1e-3
    a = np.zeros((E, N, 2), np.float32)
    a[..., 0] = 0.01
    return dict(E=E, N=N, xy=xy, th=th, actions=a, steps=2, objects=np.tile(scenes.CFG4_OBJECTS[None], (E, 1, 1)), kw=scenes.compound_kw())


def test_compound_scene_needs_the_fixture_to_body_table():
    sc = compound_scene()
    _, o = cs.oracle_run(sc)
    fb = cs.fixture_body(o.cfg)
    assert fb == [0, 1, 2, 0, 2, 3, 2] and fb != list(range(7))
    for e in range(sc['E']):        # on the oracle: kilobot 0 holds two entries of object 0, through fixtures 0 and 3
        mine = [(c, f) for c, f, _, _ in ref.env_lists(o.ws_cnt[e], o.ws_key[e], o.ws_acc[e], o.cap, sc['N'], fb)[0]]
        assert mine == [(sc['N'] + 4, 0), (sc['N'] + 4, 3)], mine
    g = run(sc)
    assert_ws_same(o, g, 'compound')
    p, i, t, ob = check(g, (1, 2, 0, 8), 'compound')
    N = sc['N']
    assert p[:, 0, :3].tolist() == [[N + 4, N + 4, -1]] * 2 and (i[:, 0, :2] > 0).all() and (t[:, 0, 2] == 2).all()
    assert p[:, 1, 0].tolist() == [N + 5] * 2 and p[:, 2, 0].tolist() == [N + 7] * 2      # fixture 1 -> disc, fixture 5 -> the box: object 3
    assert ob[..., 0].tolist() == [[2, 1, 0, 1]] * 2
    assert p[:, 3, 0].tolist() == [4, 4] and p[:, 4, 0].tolist() == [3, 3]


def test_null_combinations_prefilled_and_reused_outputs_and_a_side_stream():
    sc = cs.s1()
    g = run(sc)
    E, N, M = sc['E'], sc['N'], 1
    exp = {k: want(g, k) for k in (0, 3, 8)}
    lib, h = g._lib, g._h
    import ctypes as C
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    for k in (3, 8):
        for lists in (True, False):
            for touch in (True, False):
                for obj in (True, False):
                    if not (lists or touch or obj):
                        continue
                    p = torch.full((E, N, k), 7, dtype=torch.int32, device='cuda') if lists else None
                    i = torch.full((E, N, k), NAN, device='cuda') if lists else None
                    t = torch.full((E, N, 4), NAN, device='cuda') if touch else None
                    o = torch.full((E, M, 2), NAN, device='cuda') if obj else None
                    assert lib.kb_sense_contacts(h, k, 65536.0, ptr(p), ptr(i), ptr(t), ptr(o), None) == 0
                    x = exp[k]
                    same((p, i, t, o), (x[0] if lists else None, x[1] if lists else None, x[2] if touch else None, x[3] if obj else None),
                         'k %d lists %d touch %d obj %d' % (k, lists, touch, obj))
    # out=: NaN-prefilled tensors are overwritten everywhere, and again after the store has changed
    out = (torch.full((E, N, 8), -5, dtype=torch.int32, device='cuda'), torch.full((E, N, 8), NAN, device='cuda'),
           torch.full((E, N, 4), NAN, device='cuda'), torch.full((E, M, 2), NAN, device='cuda'))
    got = g.contacts(8, out=out)
    assert all(a is b for a, b in zip(got, out))
    same(got, exp[8], 'out=')
    agg = g.contacts(0, out=(out[2], out[3]))
    assert agg[0] is None and agg[1] is None and agg[2] is out[2]
    same(agg, exp[0], 'out= aggregate only')
    g.step(10, actions=dev(sc['actions']))
    same(g.contacts(8, out=out), want(g, 8), 'out= reused')
    with pytest.raises(ValueError):
        g.contacts(8, out=out[:3])
    with pytest.raises(ValueError):
        g.contacts(17)
    with pytest.raises(ValueError):
        g.contacts(8, scale=0.0)
    # another scale; unaligned rows (k = 3) were covered above
    same(g.contacts(8, scale=1000.0), want(g, 8, 1000.0), 'scale 1000')
    # a side stream gives the default stream's answer
    full = g.contacts(8)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        s = g.contacts(8)
    side.synchronize()
    same(s, tuple(None if t is None else cpu(t) for t in full), 'side stream')


def test_state_and_store_are_untouched():
    sc = cs.s1()
    g = run(sc)
    fields = ('x', 'y', 'theta', 'ox', 'oy', 'otheta', 'ovx', 'ovy', 'ow', 'v', 'w', 'status', 'ws_cnt', 'ws_key', 'ws_acc', 'ows_acc')
    torch.cuda.synchronize()
    kept = {f: getattr(g, f).clone() for f in fields}
    for k in (8, 16, 0):
        g.contacts(k)
    torch.cuda.synchronize()
    for f in fields:
        assert torch.equal(kept[f].view(torch.uint8), getattr(g, f).view(torch.uint8)), f
    # ... and the next step does not see that the slice of scratch was used: the same poses as a sim that never sensed
    twin = run(sc)
    for s in (g, twin):
        s.step(10, actions=dev(sc['actions']))
    torch.cuda.synchronize()
    for f in ('x', 'y', 'theta', 'ws_acc'):
        assert torch.equal(getattr(g, f), getattr(twin, f)), f


def test_shard_equals_rows_of_the_unsharded_batch():
    E, N = 8, 96
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.08, seed=31)
    a = np.zeros((E, N, 2), np.float32)
    a[..., 0] = 0.01
    sl = slice(3, 6)
    full, part = make_sim(E, N, xy, th), make_sim(3, N, xy[sl], th[sl])
    for s, rows in ((full, slice(None)), (part, sl)):
        s.step(1, flags=cs.STEP_NO_DRIVE)
        for _ in range(2):
            s.step(10, actions=dev(a[rows]))
    f, p = full.contacts(8), part.contacts(8)
    torch.cuda.synchronize()
    assert cpu(p[2])[..., 0].sum() > 100
    same(p, tuple(None if t is None else cpu(t)[sl] for t in f), 'shard')
    check(part, (8,), 'shard against the restatement')


def test_entries_of_sleeping_islands_persist():
    """allow_sleep = 1: S2 driven for three steps, then left alone until islands fall asleep (their velocities decay below
    Box2D's tolerances for half a second); the store keeps the contacts of a sleeping island, and they are reported."""
    sc = cs.s2()
    g = run(sc, allow_sleep=1)
    for _ in range(10):
        g.step(10, actions=torch.zeros(sc['E'], sc['N'], 2, device='cuda'))
    p, i, t, o = check(g, (8, 0), 'sleeping')
    asleep = cpu(g.sleep_time) < 0
    assert asleep.sum() > 100 and (t[..., 0][asleep] > 0).sum() > 100
    g.step(10)      # asleep: the entries are still there after another step
    p2, i2, t2, o2 = check(g, (8,), 'still sleeping')
    assert (t2[..., 0][cpu(g.sleep_time) < 0] > 0).sum() > 100


def test_batched_env_contact_obs():
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    E, N = 3, 64
    kw = dict(num_objects=1, obj_radius=[0.075])
    env = BatchedKilobotsEnv(E, N, seed=3, spawn_std=0.08, contact_obs=8, **kw)
    plain = BatchedKilobotsEnv(E, N, seed=3, spawn_std=0.08, contact_obs=None, **kw)
    for e in (env, plain):
        e.sim.set_objects_m(np.tile(np.array([[0.05, 0.0]])[None], (E, 1, 1)))
    assert torch.equal(env.reset(), plain.reset())
    a = torch.zeros(E, N, 2, device='cuda')
    a[..., 0] = 0.01
    obs, _, _, info = env.step(a)
    pobs, _, _, pinfo = plain.step(a)
    assert pinfo == {} and torch.equal(obs, pobs)
    assert sorted(info) == ['contacts'] and len(info['contacts']) == 4
    direct = env.sim.contacts(8)
    exp = tuple(cpu(t) for t in direct)
    same(info['contacts'], exp, 'info')
    same(env.contacts(), exp, 'env.contacts()')
    same(direct, want(env.sim, 8), 'restatement')
    assert exp[2][..., 0].sum() > 20
    with pytest.raises(ValueError):
        plain.contacts()
    bare = BatchedKilobotsEnv(2, 16, seed=3, contact_obs=0)
    bare.reset()
    c = bare.step(torch.zeros(2, 16, 2, device='cuda'))[3]['contacts']
    assert c[0] is None and c[1] is None and c[3] is None and tuple(c[2].shape) == (2, 16, 4)
