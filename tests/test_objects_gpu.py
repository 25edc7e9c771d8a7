"""kb_sense_objects on the GPU against the numpy restatement of its definition (tests/objects_ref.py), whose geometry comes
from kb_get_outline alone.

Everything is compared for equality of the bit patterns: every operation of the definition is one fp32 operation rounded
on its own, on the device and in the restatement.  No tolerances."""
import numpy as np
import pytest
import torch

from tests import objects_ref as ref
from tests import scenes
from tests.gpu_common import Spy, cpu, dev, same_as_f32 as same
from tests.sensing_common import make_sim

pytestmark = pytest.mark.gpu

NAN = float('nan')
STATE = ('x', 'y', 'theta', 'ox', 'oy', 'otheta')
SETS = ref.object_sets()


def make(E, N, name, seed):
    kw, centres = SETS[name]
    xy, th, objs, oth = ref.spawn_over_objects(E, N, centres, seed)
    g = make_sim(E, N, xy, th, **kw)
    g.set_objects_m(objs, oth)
    return g


def want(g):
    """The restatement on the state of the sim as it is on the device: (obj, wall, [aux per env])."""
    torch.cuda.synchronize()
    s = [cpu(getattr(g, f)) if getattr(g, f) is not None else None for f in STATE]
    return ref.restate(ref.tables(g.outline()), *s)


def check(g, what=''):
    wobj, wwall, aux = want(g)
    obj, wall = g.object_points()
    torch.cuda.synchronize()
    E, N, M = g.num_envs, g.num_bots, g.num_objects
    assert obj.dtype == wall.dtype == torch.float32 and tuple(obj.shape) == (E, N, M, 4) and tuple(wall.shape) == (E, N, 4)
    dobj, dwall = ref.bits(cpu(obj)) != ref.bits(wobj), ref.bits(cpu(wall)) != ref.bits(wwall)
    print('%s E=%d N=%d M=%d: %d of %d object words and %d of %d wall words differ; %d rows inside, %d ties'
          % (what, E, N, M, int(dobj.sum()), dobj.size, int(dwall.sum()), dwall.size, int(wobj[..., 3].sum()), sum(int((a['ties'] > 1).sum()) for a in aux)))
    assert not dobj.any(), (what, np.argwhere(dobj)[:5])
    assert not dwall.any(), (what, np.argwhere(dwall)[:5])
    return wobj, wwall, aux


@pytest.mark.parametrize('name', ['disc', 'boxes', 'mixed', 'forms'])
@pytest.mark.parametrize('E,N', [(5, 1), (2, 7), (8, 64), (3, 333), (2, 1024)])
def test_object_points_equal_the_restatement(E, N, name):
    """One kilobot, a partial wave, one wave, a partial tile behind a full one, four full tiles; one disc, four rotated boxes,
    eight mixed objects, the 8-fixture LForm / TForm / CForm / disc scene.  Random headings; the kilobots are drawn around
    the objects, so that some are inside."""
    g = make(E, N, name, seed=E * N)
    wobj, wwall, _ = check(g, name)
    if E * N >= 64:
        assert 0 < wobj[..., 3].sum() < wobj[..., 3].size       # some inside, some outside
    assert (wwall[..., 2] > 0).all()


def test_constructed_cases():
    """One env of 64: an axis-aligned box of half extents (2, 1) at the origin, a disc of radius 2 at (12.5, 0), a CForm at
    (-12.5, 0), world units; the first kilobots sit on the special points, the rest around the objects.  Every case is
    asserted on the restatement (the tie, the clamp, the inside flag) before the device is compared with it."""
    cf = scenes.reference_polygon_fixtures(scenes.CFORM)
    kw = ref.fixtures_kw(3, [(1, [[2.0, 1.0]], 0, 0.0), (0, None, 1, 0.08), (2, cf[0], 2, 0.0), (2, cf[1], 2, 0.0), (2, cf[2], 2, 0.0)])
    N = 64
    g = make_sim(1, N, **kw)
    tab = ref.tables(g.outline())
    arm = tab['fixtures'][4]['verts'].astype(np.float64)        # the upper arm of the C: its inner corner is its rightmost low vertex
    corner = arm[np.lexsort((arm[:, 1], -arm[:, 0]))[0]] + np.array([-12.5, 0.0])
    cases = [
        ('diagonal', (1.5, -0.5)), ('on an edge', (0.5, -1.0)), ('on a vertex', (2.0, -1.0)), ('beyond a vertex, at b', (3.0, -2.0)),
        ('beyond a vertex, at a', (-3.0, -2.0)), ('inside the box', (0.25, 0.125)), ('inside the disc', (13.0, 0.5)),
        ('disc centre', (12.5, 0.0)), ('cavity of the C', tuple(corner + [-0.3, -0.3])), ('inside the C at its inner corner', tuple(corner + [0.2, 0.2])),
        ('on a wall', (-25.0, 3.0)), ('outside the arena', (26.0, 0.5)), ('two walls', (-22.0, -15.75)), ('beyond a corner of the arena', (-26.0, -20.0)),
    ]
    rng = np.random.RandomState(5)
    xy = np.concatenate([np.array([c for _, c in cases]), rng.normal(scale=2.0, size=(N - len(cases), 2)) + np.array([[0.0, 0.0], [12.5, 0.0], [-12.5, 0.0]])[rng.randint(0, 3, N - len(cases))]])
    g.x.copy_(dev(xy[None, :, 0].astype(np.float32)))
    g.y.copy_(dev(xy[None, :, 1].astype(np.float32)))
    g.theta.copy_(dev(rng.uniform(-np.pi, np.pi, size=(1, N)).astype(np.float32)))
    g.ox.copy_(dev(np.array([[0.0, 12.5, -12.5]], dtype=np.float32)))
    g.oy.zero_()
    g.otheta.zero_()
    wobj, wwall, (aux,) = check(g, 'constructed')
    i = {name: k for k, (name, _) in enumerate(cases)}
    o, w = wobj[0], wwall[0]
    k = i['diagonal']       # the bottom and the right edge tie: the lower one wins
    assert aux['ties'][k, 0] == 2 and aux['winner'][k, 0] == 0 and o[k, 0, 3] == 1 and o[k, 0, 2] == np.float32(0.5) / np.float32(25)
    k = i['on an edge']
    assert o[k, 0, 2] == 0 and aux['winner'][k, 0] == 0 and not aux['lo'][k, 0] and not aux['hi'][k, 0] and o[k, 0, 3] == 1
    k = i['on a vertex']
    assert o[k, 0, 2] == 0 and aux['ties'][k, 0] == 2 and aux['winner'][k, 0] == 0 and aux['hi'][k, 0]
    k = i['beyond a vertex, at b']
    assert aux['hi'][k, 0] and aux['ties'][k, 0] == 2 and aux['winner'][k, 0] == 0 and o[k, 0, 3] == 0
    k = i['beyond a vertex, at a']
    assert aux['lo'][k, 0] and aux['ties'][k, 0] == 2 and aux['winner'][k, 0] == 0 and o[k, 0, 3] == 0
    k = i['inside the box']
    assert o[k, 0, 3] == 1 and aux['winner'][k, 0] == 2 and aux['ties'][k, 0] == 1
    k = i['inside the disc']
    assert o[k, 1, 3] == 1 and o[k, 1, 2] > 0 and o[k, 0, 3] == 0
    k = i['disc centre']
    assert o[k, 1, 3] == 1 and o[k, 1, 2] == tab['fixtures'][1]['radius'] / np.float32(25)
    k = i['cavity of the C']      # outside, the spine and the arm about equally near
    assert o[k, 2, 3] == 0 and o[k, 2, 2] * 25 < 0.31 and aux['second'][k, 2] - o[k, 2, 2] * 25 < 0.1
    k = i['inside the C at its inner corner']
    assert o[k, 2, 3] == 1 and 0 < o[k, 2, 2] * 25 < 0.21
    k = i['on a wall']
    assert w[k, 2] == 0 and w[k, 3] == 0
    k = i['outside the arena']
    assert w[k, 2] == np.float32(-1) / np.float32(25) and w[k, 3] == 1
    k = i['two walls']
    assert aux['walltie'][k] == 2 and w[k, 3] == 0 and w[k, 2] == np.float32(3) / np.float32(25)
    k = i['beyond a corner of the arena']      # the most negative gap wins
    assert w[k, 3] == 2 and w[k, 2] == np.float32(-1.25) / np.float32(25)


def test_after_motion_and_untouched_state():
    """64 velocity kilobots push four boxes for 20 steps of 10 substeps; then the points are those of the restatement on the
    state the step left, and sensing changes no state tensor."""
    E, N = 2, 64
    kw, centres = SETS['boxes']
    xy, _ = scenes.gaussian_spawn(E, N, sigma=0.3, seed=63)
    g = make_sim(E, N, xy, scenes.toward_objects_theta(xy), **kw)
    objs = np.tile(centres[None], (E, 1, 1))
    g.set_objects_m(objs, np.tile(np.array([0.4, 0.0, -1.2, 0.8])[None], (E, 1)))
    a = torch.zeros(E, N, 2, device='cuda')
    a[..., 0] = 0.01
    for _ in range(20):
        g.step(10, actions=a)
    torch.cuda.synchronize()
    assert float((g.object_poses()[..., :2] - dev(objs.astype(np.float32))).abs().max()) > 1e-4       # the boxes were pushed
    fields = STATE + ('ovx', 'ovy', 'ow', 'v', 'w', 'status', 'ws_cnt', 'ows_acc')
    before = {f: getattr(g, f).clone() for f in fields}
    check(g, 'after motion')
    torch.cuda.synchronize()
    for f in fields:
        assert torch.equal(before[f].view(torch.uint8), getattr(g, f).view(torch.uint8)), f


def test_outputs_streams_and_arguments():
    E, N = 3, 333
    g = make(E, N, 'forms', seed=8)
    M = g.num_objects
    wobj, wwall, _ = want(g)
    # buffers full of NaN come back fully written; reused: the same answer twice
    obj, wall = torch.full((E, N, M, 4), NAN, device='cuda'), torch.full((E, N, 4), NAN, device='cuda')
    for _ in range(2):
        got = g.object_points(out=(obj, wall))
        assert got[0].data_ptr() == obj.data_ptr() and got[1].data_ptr() == wall.data_ptr()
        assert same(obj, wobj) and same(wall, wwall)
    # walls=False hands the library NULL for d_wall and returns obj alone
    spy = Spy(g._lib)
    g._lib = spy
    try:
        only = g.object_points(walls=False)
        obj.fill_(NAN)
        into = g.object_points(out=obj, walls=False)
        g.object_points()
    finally:
        g._lib = spy.lib
    calls = [a for n, a in spy.calls if n == 'kb_sense_objects']
    assert len(calls) == 3 and [c[2] is None for c in calls] == [True, True, False] and all(c[1] is not None for c in calls)
    assert torch.is_tensor(only) and same(only, wobj) and into.data_ptr() == obj.data_ptr() and same(obj, wobj)
    # a side stream gives the default stream's answer
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        so, sw = g.object_points()
    side.synchronize()
    assert same(so, wobj) and same(sw, wwall)
    # arguments are checked before the call
    spy = Spy(g._lib)
    g._lib = spy
    try:
        for bad in (obj, (obj,), (wall, obj), (obj, wall.double()), (obj.cpu(), wall), (obj.view(E, N, M * 4), wall), (obj[:2], wall[:2]),
                    (obj, wall, wall), (obj.transpose(0, 1), wall), (obj, torch.zeros(E * N * 4 + 1, device='cuda')[1:].view(E, N, 4))):
            with pytest.raises(ValueError):
                g.object_points(out=bad)
        for bad in (wall, (obj, wall), obj[..., :3]):
            with pytest.raises(ValueError):
                g.object_points(out=bad, walls=False)
    finally:
        g._lib = spy.lib
    assert not spy.calls


def test_a_sim_without_objects_returns_the_walls_only():
    E, N = 2, 96
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.3, seed=9)
    g = make_sim(E, N, xy, th)
    assert g.num_objects == 0 and g.outline().num_fixtures == 0
    _, wwall, _ = want(g)
    wall = g.object_points()
    assert torch.is_tensor(wall) and tuple(wall.shape) == (E, N, 4) and same(wall, wwall)
    buf = torch.full((E, N, 4), NAN, device='cuda')
    assert g.object_points(out=buf).data_ptr() == buf.data_ptr() and same(buf, wwall)
    with pytest.raises(ValueError):
        g.object_points(walls=False)
    with pytest.raises(ValueError):
        g.object_points(out=(torch.zeros(E, N, 0, 4, device='cuda'), buf))


def test_a_shard_reproduces_its_rows():
    E, N = 4, 64
    kw, centres = SETS['mixed']
    xy, th, objs, oth = ref.spawn_over_objects(E, N, centres, seed=6)
    whole, shard = make_sim(E, N, xy, th, **kw), make_sim(2, N, xy[2:4], th[2:4], **kw)
    whole.set_objects_m(objs, oth)
    shard.set_objects_m(objs[2:4], oth[2:4])
    ow, ww = whole.object_points()
    os_, ws = shard.object_points()
    assert torch.equal(ow[2:4].contiguous().view(torch.int32), os_.view(torch.int32))
    assert torch.equal(ww[2:4].contiguous().view(torch.int32), ws.view(torch.int32))
    assert bool(os_[..., 3].any())


def test_batched_env_object_obs():
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    E, N = 4, 64
    kw, centres = SETS['boxes']
    objs = np.tile(centres[None], (E, 1, 1))
    env = BatchedKilobotsEnv(E, N, seed=3, spawn_std=0.12, object_obs=True, **kw)
    plain = BatchedKilobotsEnv(E, N, seed=3, spawn_std=0.12, **kw)
    for e in (env, plain):
        e.sim.set_objects_m(objs)
    assert torch.equal(env.reset(), plain.reset())
    a = dev(scenes.random_actions(E, N, seed=20))
    obs, _, _, info = env.step(a)
    pobs, _, _, pinfo = plain.step(a)
    assert pinfo == {} and torch.equal(obs, pobs)
    assert sorted(info) == ['objects', 'walls']
    obj, wall = env.sim.object_points()
    assert torch.equal(info['objects'].view(torch.int32), obj.view(torch.int32)) and torch.equal(info['walls'].view(torch.int32), wall.view(torch.int32))
    mobj, mwall = env.object_points()
    assert torch.equal(mobj.view(torch.int32), obj.view(torch.int32)) and torch.equal(mwall.view(torch.int32), wall.view(torch.int32))
    wobj, wwall, _ = want(env.sim)
    assert same(obj, wobj) and same(wall, wwall)
    with pytest.raises(ValueError):
        plain.object_points()
    bare = BatchedKilobotsEnv(2, 16, seed=3, object_obs=True)
    bare.reset()
    info = bare.step(dev(scenes.random_actions(2, 16, seed=21)))[3]
    assert sorted(info) == ['walls'] and same(info['walls'], want(bare.sim)[1])
