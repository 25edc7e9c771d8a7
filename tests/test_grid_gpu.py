"""kb_sense_grid on the GPU against the numpy restatement of its definition (tests/grid_ref.py), whose arena and fixtures
come from kb_get_outline alone and whose object masks are the inside flag of tests/objects_ref.py.

Everything is compared for equality of the bit patterns: every operation of the definition is one fp32 operation rounded
on its own, the sums are integer sums, on the device and in the restatement.  No tolerances."""
import numpy as np
import pytest
import torch

from gym_kilobots_amd import _native as nat
from tests import grid_ref as ref
from tests import objects_ref
from tests import scenes
from tests.gpu_common import cpu, dev, object_state as state, same_as_f32 as same
from tests.sensing_common import f32, make_sim

pytestmark = pytest.mark.gpu

NAN = float('nan')
STATE = ('x', 'y', 'theta', 'ox', 'oy', 'otheta')
SETS = objects_ref.object_sets()
# one cell; odd sizes on the scalar store path; one band; several bands with a partial last band (127 x 95 with the flow:
# 32 + 32 + 31 rows) and a partial last tile of cells; the largest grid (with the flow four bands, the count alone one of 64 KiB)
GRIDS = [(1, 1), (3, 2), (7, 5), (64, 48), (127, 95), (128, 128)]
BOTS = ref.COUNT | ref.FLOW


def want(g, gw, gh, planes):
    """The restatement on the state of the sim as it is on the device."""
    return ref.restate(objects_ref.tables(g.outline()), gw, gh, planes, *state(g))


def check(g, gw, gh, planes, what='', w=None):
    w = want(g, gw, gh, planes) if w is None else w
    got = g.occupancy_grid(gw, gh, planes)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == w.shape and got.is_contiguous()
    d = ref.bits(cpu(got)) != ref.bits(w)
    print('%s E=%d N=%d %d x %d planes %d: %d of %d words differ' % (what, g.num_envs, g.num_bots, gw, gh, planes, int(d.sum()), d.size))
    assert not d.any(), (what, gw, gh, planes, np.argwhere(d)[:5])
    return w


def make_objects(E, N, name, seed):
    kw, centres = SETS[name]
    xy, th, objs, oth = objects_ref.spawn_over_objects(E, N, centres, seed)
    g = make_sim(E, N, xy, th, **kw)
    g.set_objects_m(objs, oth)
    return g


@pytest.mark.parametrize('scene', ['gaussian', 'disc', 'boxes', 'mixed', 'forms'])
@pytest.mark.parametrize('E,N', [(5, 1), (2, 7), (8, 64), (3, 333), (2, 1024)])
def test_grids_equal_the_restatement(E, N, scene):
    """Every grid of GRIDS on one sim per case.  'gaussian': a Gaussian spawn with random headings, the count alone and
    count + flow.  The object sets (one disc, four rotated boxes, eight mixed objects, the 8-fixture LForm / TForm / CForm /
    disc scene): all three planes, the kilobots drawn around the objects; from 64 x 48 upward every object plane has both
    ones and zeros."""
    if scene == 'gaussian':
        xy, th = scenes.gaussian_spawn(E, N, sigma=0.2, seed=E * N)
        g = make_sim(E, N, xy, th)
    else:
        g = make_objects(E, N, scene, seed=E * N + 1)
    for gw, gh in GRIDS:
        if scene == 'gaussian':
            w = check(g, gw, gh, BOTS, scene)
            check(g, gw, gh, ref.COUNT, scene, w[:, :1])
        else:
            w = check(g, gw, gh, ref.ALL, scene)
            if gw >= 64:
                masks = w[:, 3:]
                assert (masks.max((2, 3)) == 1).all() and (masks.min((2, 3)) == 0).all()
        assert (w[:, 0].sum((1, 2), dtype=np.float64) == N).all()


def test_constructed_cases():
    """One env of 64 on a 50 x 75 grid, whose cells are 1 x 0.5 world units and whose constants are exact in fp32 (icw = 1,
    ich = 2): the first kilobots sit on the special points, the rest in a corner of their own.  Every case is asserted on the
    restatement before the device is compared with it."""
    N, gw, gh = 64, 50, 75
    g = make_sim(1, N)
    tab = objects_ref.tables(g.outline())
    assert tab['arena'].tolist() == [-25.0, 25.0, -18.75, 18.75]
    th0 = 0.7
    cases = [    # (name, x, y, theta, expected (ix, iy))
        ('on an interior column boundary', -25.0 + 7.0, 3.3, 0.1, (7, 44)), ('on an interior row boundary', -3.25, -18.75 + 11.0, 0.2, (21, 22)),
        ('on an interior corner', -25.0 + 30.0, -18.75 + 5.5, 0.3, (30, 11)),
        ('on xmin', -25.0, 1.3, 0.4, (0, 40)), ('on xmax', 25.0, 1.3, 0.5, (49, 40)), ('on ymin', 2.5, -18.75, 0.6, (27, 0)), ('on ymax', 2.5, 18.75, 0.7, (27, 74)),
        ('left of the arena', -26.0, -1.3, 0.8, (0, 34)), ('right of the arena', 27.5, -1.3, 0.9, (49, 34)), ('below the arena', -2.5, -20.0, 1.0, (22, 0)),
        ('above the arena', -2.5, 40.0, 1.1, (22, 74)), ('beyond a corner', 26.0, 20.0, 1.2, (49, 74)), ('beyond the opposite corner', -1e9, -1e9, 1.3, (0, 0)),
        ('a NaN x', NAN, 5.1, 1.4, (0, 47)),
        ('pair, heading t', 10.25, 10.1, th0, (35, 57)), ('pair, heading t + pi', 10.75, 10.2, float(np.float32(th0) + np.float32(np.pi)), (35, 57)),
    ]
    rng = np.random.RandomState(5)
    k = len(cases)
    x = np.concatenate([[c[1] for c in cases], rng.uniform(-20.0, -10.0, N - k)])
    y = np.concatenate([[c[2] for c in cases], rng.uniform(-15.0, -5.0, N - k)])
    th = np.concatenate([[c[3] for c in cases], rng.uniform(-np.pi, np.pi, N - k)])
    g.x.copy_(dev(f32(x[None])))
    g.y.copy_(dev(f32(y[None])))
    g.theta.copy_(dev(f32(th[None])))
    ix, iy = ref.cells(tab, gw, gh, f32(x), f32(y))
    for j, (name, _, _, _, cell) in enumerate(cases):
        assert (ix[j], iy[j]) == cell, name
    w = ref.restate(tab, gw, gh, BOTS, f32(x[None]), f32(y[None]), f32(th[None]))
    assert w[0, 0].sum() == N
    alone = [j for j in range(k - 2) if cases[j][4] not in [c[4] for c in cases[:j] + cases[j + 1:]]]
    assert len(alone) == k - 2
    for j in alone:       # a lone kilobot's cell holds 1 and its own quantised heading
        s, c = objects_ref.O.sincosf(float(np.float32(th[j])))
        q = ref.reduce_ref.quant(f32([c, s]), 65536.0).astype(np.float32) / np.float32(65536)
        assert w[0, :, iy[j], ix[j]].tolist() == [1.0, q[0], q[1]], cases[j][0]
    # the pair: its count is 2, its flow whatever the quantised sum says (cos and sin of t + pi are not minus those of t to the bit)
    qc, qs = ref.quantised_headings(f32(th[k - 2:k]))
    assert w[0, 0, 57, 35] == 2
    assert w[0, 1, 57, 35] == np.float32(int(qc.sum())) / np.float32(65536) and w[0, 2, 57, 35] == np.float32(int(qs.sum())) / np.float32(65536)
    print('the pair of opposite headings sums to (%d, %d) / 65536' % (qc.sum(), qs.sum()))
    assert abs(int(qc.sum())) <= 2 and abs(int(qs.sum())) <= 2
    check(g, gw, gh, BOTS, 'constructed', w)
    for gw2, gh2 in ((7, 5), (128, 128)):       # the same kilobots on grids whose constants are rounded
        check(g, gw2, gh2, BOTS, 'constructed')


def test_all_kilobots_of_an_env_in_one_cell():
    """1024 adds on one LDS word (three with the flow) serialise and stay correct, while a second env is spread out."""
    E, N, gw, gh = 2, 1024, 128, 128
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.3, seed=77)
    xy[0] = np.array([0.1333, -0.0871]) + np.random.RandomState(2).uniform(-0.002, 0.002, size=(N, 2))
    g = make_sim(E, N, xy, th)
    w = want(g, gw, gh, BOTS)
    assert w[0, 0].max() == N and (w[0, 0] > 0).sum() == 1 and w[1, 0].max() < 64
    assert (w[0, 1:] != 0).sum() == 2       # (1024 random headings: neither sum vanishes)
    check(g, gw, gh, BOTS, 'one cell', w)
    check(g, gw, gh, ref.COUNT, 'one cell', w[:, :1])


def test_object_planes_equal_the_inside_flag_of_object_points():
    """Device against device: 1024 kilobots on the fp32 cell centres of a 32 x 32 grid with theta = 0.  The object planes are
    the fourth word of kb_sense_objects' rows bit for bit; every cell counts one kilobot heading along x."""
    E, gw, gh = 2, 32, 32
    N = gw * gh
    for name in ('mixed', 'forms'):
        kw, centres = SETS[name]
        _, _, objs, oth = objects_ref.spawn_over_objects(E, 1, centres, seed=17)
        g = make_sim(E, N, **kw)
        g.set_objects_m(objs, oth)
        cx, cy = ref.centres(objects_ref.tables(g.outline()), gw, gh)
        g.x.copy_(dev(np.tile(cx[None], (E, 1))))
        g.y.copy_(dev(np.tile(cy[None], (E, 1))))
        g.theta.zero_()
        grid = g.occupancy_grid(gw, gh, ref.ALL)
        obj = g.object_points(walls=False)
        torch.cuda.synchronize()
        M = g.num_objects
        flags = obj[..., 3].permute(0, 2, 1).reshape(E, M, gh, gw).contiguous()
        assert torch.equal(grid[:, 3:].contiguous().view(torch.int32), flags.view(torch.int32)), name
        assert bool((flags.amax((2, 3)) == 1).all()) and bool((flags.amin((2, 3)) == 0).all())
        assert bool((grid[:, 0] == 1).all()) and bool((grid[:, 1] == 1).all()) and not bool(grid[:, 2].view(torch.int32).any())


def test_every_element_is_written():
    """out= full of NaN comes back without one, on the 16-byte store path, on the scalar one (an odd width; a width of 4 k on
    a buffer that is only float aligned) and with planes that take two launches; the same tensor is returned."""
    E, N = 3, 333
    g = make_objects(E, N, 'boxes', seed=4)
    C = g.grid_channels(ref.ALL)
    assert C == 3 + g.num_objects
    for gw, gh in ((64, 48), (7, 5), (127, 95), (128, 128)):
        w = want(g, gw, gh, ref.ALL)
        n = E * C * gh * gw
        for off in (0, 1):
            buf = torch.full((n + off,), NAN, device='cuda')
            out = buf[off:].view(E, C, gh, gw)
            assert (out.data_ptr() % 16 == 0) == (off == 0)
            for _ in range(2):      # reused: the same answer twice
                got = g.occupancy_grid(gw, gh, ref.ALL, out=out)
                assert got.data_ptr() == out.data_ptr()
                assert not bool(torch.isnan(out).any()) and same(out, w)
        sub = torch.full((E, 2, gh, gw), NAN, device='cuda')
        g.occupancy_grid(gw, gh, ('flow',), out=sub)
        assert not bool(torch.isnan(sub).any()) and same(sub, w[:, 1:3])
    for bad in (torch.zeros(E, C, 48, 64), torch.zeros(E, C, 64, 48, device='cuda'), torch.zeros(E, C - 1, 48, 64, device='cuda'),
                torch.zeros(E, C, 48, 64, device='cuda', dtype=torch.float64), torch.zeros(E, C, 64, 48, device='cuda').transpose(2, 3)):
        with pytest.raises(ValueError):
            g.occupancy_grid(64, 48, ref.ALL, out=bad)
    plain = make_sim(2, 16)
    with pytest.raises(ValueError):
        plain.occupancy_grid(8, 8, ('count', 'objects'))
    with pytest.raises(ValueError):
        plain.grid_channels(nat.GRID_OBJECTS)
    assert plain.grid_channels() == 1 and tuple(plain.occupancy_grid(8, 6).shape) == (2, 1, 6, 8)


def test_after_motion_and_untouched_state():
    """64 velocity kilobots push four boxes for 20 steps of 10 substeps; the grid taken before no longer holds, the one taken
    after is the restatement on the state the step left, and sensing changes no state tensor."""
    E, N, gw, gh = 2, 64, 64, 48
    kw, centres = SETS['boxes']
    xy, _ = scenes.gaussian_spawn(E, N, sigma=0.3, seed=63)
    g = make_sim(E, N, xy, scenes.toward_objects_theta(xy), **kw)
    g.set_objects_m(np.tile(centres[None], (E, 1, 1)), np.tile(np.array([0.4, 0.0, -1.2, 0.8])[None], (E, 1)))
    before = check(g, gw, gh, ref.ALL, 'before motion')
    a = torch.zeros(E, N, 2, device='cuda')
    a[..., 0] = 0.01
    for _ in range(20):
        g.step(10, actions=a)
    fields = STATE + ('ovx', 'ovy', 'ow', 'v', 'w', 'status', 'ws_cnt', 'ows_acc')
    torch.cuda.synchronize()
    kept = {f: getattr(g, f).clone() for f in fields}
    after = check(g, gw, gh, ref.ALL, 'after motion')
    assert (before[:, 0] != after[:, 0]).any()       # the kilobots have moved on by several cells
    torch.cuda.synchronize()
    for f in fields:
        assert torch.equal(kept[f].view(torch.uint8), getattr(g, f).view(torch.uint8)), f


def test_plane_subsets_are_slices_of_the_full_call():
    E, N = 3, 333
    g = make_objects(E, N, 'forms', seed=8)
    tab = objects_ref.tables(g.outline())
    for gw, gh in ((7, 5), (64, 48), (127, 95)):
        full = g.occupancy_grid(gw, gh, ref.ALL)
        at = ref.plane_slices(tab, ref.ALL)
        for planes, names in ((1, ('count',)), (2, ('flow',)), (3, ('count', 'flow')), (4, ('objects',)), (5, ('objects', 'count')),
                              (6, ('flow', 'objects')), (7, ('count', 'flow', 'objects'))):
            part = g.occupancy_grid(gw, gh, planes)
            assert part.shape[1] == g.grid_channels(planes) == ref.channels(tab, planes)
            for bit, sl in ref.plane_slices(tab, planes).items():
                assert torch.equal(part[:, sl].contiguous().view(torch.int32), full[:, at[bit]].contiguous().view(torch.int32)), (gw, gh, planes, bit)
            assert torch.equal(part.view(torch.int32), g.occupancy_grid(gw, gh, names).view(torch.int32))
    # a side stream gives the default stream's answer
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        s = g.occupancy_grid(127, 95, ref.ALL)
    side.synchronize()
    assert torch.equal(s.view(torch.int32), full.view(torch.int32))


def test_batched_env_grid_obs():
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    E, N = 4, 64
    kw, centres = SETS['boxes']
    objs = np.tile(centres[None], (E, 1, 1))
    env = BatchedKilobotsEnv(E, N, seed=3, spawn_std=0.12, grid_obs=(64, 48, ('count', 'flow', 'objects')), **kw)
    plain = BatchedKilobotsEnv(E, N, seed=3, spawn_std=0.12, **kw)
    for e in (env, plain):
        e.sim.set_objects_m(objs)
    assert torch.equal(env.reset(), plain.reset())
    a = dev(scenes.random_actions(E, N, seed=20))
    obs, _, _, info = env.step(a)
    pobs, _, _, pinfo = plain.step(a)
    assert pinfo == {} and torch.equal(obs, pobs)
    assert sorted(info) == ['grid'] and tuple(info['grid'].shape) == (E, 7, 48, 64)
    grid = env.sim.occupancy_grid(64, 48, ref.ALL)
    assert torch.equal(info['grid'].view(torch.int32), grid.view(torch.int32))
    assert torch.equal(env.occupancy_grid().view(torch.int32), grid.view(torch.int32))
    assert same(grid, want(env.sim, 64, 48, ref.ALL))
    with pytest.raises(ValueError):
        plain.occupancy_grid()
    with pytest.raises(ValueError):
        BatchedKilobotsEnv(E, N, seed=3, grid_obs=(64, 48, ('objects',)))
    bare = BatchedKilobotsEnv(2, 16, seed=3, grid_obs=(8, 6))
    bare.reset()
    info = bare.step(dev(scenes.random_actions(2, 16, seed=21)))[3]
    assert sorted(info) == ['grid'] and same(info['grid'], want(bare.sim, 8, 6, ref.COUNT)) and float(info['grid'].sum()) == 2 * 16
