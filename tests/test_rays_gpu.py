"""kb_sense_rays on the GPU against the numpy restatement of its definition (tests/rays_ref.py): brute force over all pairs,
with the geometry from kb_get_outline alone.

Everything is compared for equality of the bit patterns: every operation of the definition is one fp32 operation rounded
on its own, on the device and in the restatement.  No tolerances.  The outputs are filled with a sentinel before every call:
a word that the kernel does not write shows.  That the scenes are not vacuous -- rays that hit kilobots, every wall, every
object, and nothing -- is asserted on the restatement alone in tests/test_rays_cpu.py."""
import numpy as np
import pytest
import torch

from gym_kilobots_amd import _native as nat
from tests import geometry_scenes as GS
from tests import rays_ref as ref
from tests import scenes
from tests.objects_ref import bits, tables
from tests.gpu_common import cpu, dev, geometry_pair, object_state as state
from tests.sensing_common import SWEEP, make_sim, sweep_scene, wall_scene

pytestmark = pytest.mark.gpu

NAN = float('nan')
SENTINEL = -77
STATE = ('x', 'y', 'theta', 'ox', 'oy', 'otheta')
ALL_K = (1, 3, 4, 7, 8, 16, 32)             # every instantiation, the padded ray counts, 16-byte and 4-byte stores, two passes


def default_targets(g):
    return nat.RAY_BOTS | nat.RAY_WALLS | (nat.RAY_OBJECTS if g.num_objects > 0 else 0)


def want(g, R, K, targets, envs=None):
    """The restatement on the state of the sim as it is on the device: (dist, hit) of all envs, or of those listed."""
    s = state(g)
    if envs is not None:
        s = [None if v is None else v[list(envs)] for v in s]
    return ref.restate(tables(g.outline()), *s, R, g.cfg.bot_radius, K, targets)


def check(g, R, K, targets=None, what='', wanted=None, envs=None, misalign=False):
    """One call with d_hit and one without, both into sentinel-filled tensors, against the restatement (`wanted` if the caller
    has it already).  misalign: the outputs start 4 bytes behind a 16-byte boundary, which takes the 4-byte stores."""
    E, N = g.num_envs, g.num_bots
    targets = default_targets(g) if targets is None else targets
    wd, wh = want(g, R, K, targets, envs) if wanted is None else wanted

    def buffers():
        if not misalign:
            return torch.full((E, N, K), NAN, device='cuda'), torch.full((E, N, K), SENTINEL, dtype=torch.int32, device='cuda')
        d, h = torch.full((E * N * K + 1,), NAN, device='cuda'), torch.full((E * N * K + 1,), SENTINEL, dtype=torch.int32, device='cuda')
        assert d.data_ptr() % 16 == 0 and h.data_ptr() % 16 == 0
        return d[1:].view(E, N, K), h[1:].view(E, N, K)
    dist, hit = buffers()
    got = g.rays(R, K, targets, out=(dist, hit))
    assert got[0].data_ptr() == dist.data_ptr() and got[1].data_ptr() == hit.data_ptr()
    alone, _ = buffers()
    only = g.rays(R, K, targets, out=alone, hit=False)
    assert only[1] is None and only[0].data_ptr() == alone.data_ptr()
    torch.cuda.synchronize()
    rows = slice(None) if envs is None else list(envs)
    gd, gh, ga = cpu(dist)[rows], cpu(hit)[rows], cpu(alone)[rows]
    dd, dh = bits(gd) != bits(wd), gh != wh
    print('%s E=%d N=%d K=%d R=%g targets=%d: %d of %d distances and %d of %d codes differ; %d rays on a kilobot, %d on a wall, %d on an object, %d on nothing'
          % (what, E, N, K, R, targets, int(dd.sum()), dd.size, int(dh.sum()), dh.size, int(((wh >= 0) & (wh < N)).sum()),
             int(((wh >= N) & (wh < N + 4)).sum()), int((wh >= N + 4).sum()), int((wh < 0).sum())))
    assert not dh.any(), (what, np.argwhere(dh)[:5], gh[dh][:5], wh[dh][:5])
    assert not dd.any(), (what, np.argwhere(dd)[:5], gd[dd][:5], wd[dd][:5])
    assert np.array_equal(bits(ga), bits(wd)), (what, 'without d_hit')
    return wd, wh


@pytest.mark.parametrize('E,N,R', SWEEP)
def test_rays_equal_the_restatement(E, N, R):
    """The sweep of the sensing kernels: cfg2 / cfg3 slices, odd sizes, one kilobot, radii from below a cell to beyond the
    arena.  Eight rays everywhere; on two scenes every ray count that takes another path."""
    xy, th = sweep_scene(E, N)
    g = make_sim(E, N, xy, th)
    counts = ALL_K if (E, N, R) in ((8, 64, 0.07), (3, 333, 0.034)) else (8,)
    for K in counts:
        check(g, R, K, what='sweep')
    if counts is ALL_K:
        check(g, R, 8, what='sweep, misaligned', misalign=True)
        check(g, R, 16, nat.RAY_BOTS, what='sweep, kilobots only')


@pytest.mark.parametrize('R', [0.04, 0.15])
def test_rays_at_walls_and_corners(R):
    """Kilobots in the corners and along the walls, some outside the arena, random headings: kilobots and walls, then each alone."""
    xy, th = wall_scene(random_headings=True)
    g = make_sim(4, xy.shape[1], xy, th)
    for targets in (nat.RAY_BOTS | nat.RAY_WALLS, nat.RAY_BOTS, nat.RAY_WALLS):
        _, wh = check(g, R, 8, targets, what='walls')
    assert set(wh.ravel().tolist()) - {-1} == set(range(xy.shape[1], xy.shape[1] + 4))        # (walls alone: all four)


def object_sim(name):
    kw, xy, th, objs, oth = ref.object_scene(name)
    g = make_sim(ref.OBJECT_SCENE['E'], ref.OBJECT_SCENE['N'], xy, th, **kw)
    g.set_objects_m(objs, oth)
    return g


@pytest.mark.parametrize('name', sorted(ref.OBJECT_SEEDS))
def test_rays_on_objects(name):
    """One disc, four rotated boxes, eight mixed objects, the 8-fixture LForm / TForm / CForm / disc scene; the kilobots are
    drawn around the objects, some inside.  All targets; the forms also alone."""
    g = object_sim(name)
    S = ref.OBJECT_SCENE
    _, wh = check(g, S['R'], S['K'], what=name)
    assert (wh >= S['N'] + 4).any()
    if name == 'forms':
        check(g, S['R'], S['K'], nat.RAY_OBJECTS, what='forms alone')
        check(g, S['R'], 7, nat.RAY_OBJECTS | nat.RAY_WALLS, what='forms and walls, 7 rays')


def test_after_pushing_and_untouched_state():
    """64 velocity kilobots push four boxes for 20 steps of 10 substeps; then the scan is that of the restatement on the state
    the step left, and sensing changes neither a state tensor nor the contact store."""
    E, N = 2, 64
    from tests.objects_ref import object_sets
    kw, centres = object_sets()['boxes']
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
    fields = STATE + ('ovx', 'ovy', 'ow', 'v', 'w', 'status', 'ws_cnt', 'ws_key', 'ws_acc', 'ows_acc', 'scratch')
    before = {f: getattr(g, f).clone() for f in fields}
    _, wh = check(g, 0.15, 16, what='after pushing')
    assert (wh >= N + 4).any() and ((wh >= 0) & (wh < N)).any()
    torch.cuda.synchronize()
    for f in fields:
        assert torch.equal(before[f].view(torch.uint8), getattr(g, f).view(torch.uint8)), f


def test_a_pile_in_one_cell():
    """40 kilobots on one point and 24 around it: one long chain in one cell, every origin of the pile inside 39 discs."""
    N = 64
    rng = np.random.RandomState(12)
    xy = np.zeros((1, N, 2))
    xy[0, :40] = (0.3123, -0.2011)
    xy[0, 40:] = xy[0, 0] + rng.uniform(-0.03, 0.03, size=(24, 2))
    g = make_sim(1, N, xy, rng.uniform(-np.pi, np.pi, size=(1, N)))
    for K in (8, 32):
        wd, wh = check(g, 0.07, K, what='pile')
    rb = np.float32(g.cfg.bot_radius) * np.float32(25)
    assert (wd[0, 1:40] <= rb / np.float32(25)).all() and (wh[0, 1:40] >= 0).all()


@pytest.mark.parametrize('row', GS.SENSING_ROWS, ids=lambda g: g.name)
def test_rays_off_the_default_arena(row):
    """The arenas and radii of tests/geometry_scenes.py that the sensing kernels are run on: cells of 0.875, 1.75 and 3.5,
    103 x 78 cells, grids one and two cells thin.  One env, eight rays, a radius of a cell and a half of the row's own cell."""
    _, _, g = geometry_pair(row)
    assert abs(g.cfg.bot_radius - row.r) < 1e-8
    check(g, GS.sensing_radius(row, 'cell-and-a-half'), 8, what=row.name, envs=(0,))


def test_a_shard_reproduces_its_rows():
    E, N = 4, 96
    xy, th = wall_scene(random_headings=True)
    whole, shard = make_sim(E, N, xy, th), make_sim(2, N, xy[2:4], th[2:4])
    dw, hw = whole.rays(0.1, 12)
    ds, hs = shard.rays(0.1, 12)
    assert torch.equal(dw[2:4].contiguous().view(torch.int32), ds.view(torch.int32)) and torch.equal(hw[2:4], hs)
    assert bool((hs >= 0).any()) and bool((hs < 0).any())


def test_calling_twice_gives_the_same_bits_on_any_stream():
    g = object_sim('mixed')
    S = ref.OBJECT_SCENE
    d1, h1 = g.rays(S['R'], 32)
    d2, h2 = g.rays(S['R'], 32)
    assert d1.data_ptr() != d2.data_ptr()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d3, h3 = g.rays(S['R'], 32)
    side.synchronize()
    for d, h in ((d2, h2), (d3, h3)):
        assert torch.equal(d1.view(torch.int32), d.view(torch.int32)) and torch.equal(h1, h)
    assert d1.dtype == torch.float32 and h1.dtype == torch.int32 and tuple(d1.shape) == tuple(h1.shape) == (S['E'], S['N'], 32)


def test_arguments_are_checked_before_the_call():
    E, N = 2, 16
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.1, seed=2)
    g = make_sim(E, N, xy, th)
    dist, hit = torch.zeros(E, N, 8, device='cuda'), torch.zeros(E, N, 8, dtype=torch.int32, device='cuda')
    for bad in (dist, (dist,), (hit, dist), (dist, hit.float()), (dist.cpu(), hit), (dist[..., :4], hit[..., :4]), (dist, hit, hit),
                (dist.transpose(0, 1), hit)):
        with pytest.raises(ValueError):
            g.rays(0.1, 8, out=bad)
    for bad in ((dist, hit), hit):
        with pytest.raises(ValueError):
            g.rays(0.1, 8, out=bad, hit=False)
    for args in ((0.0, 8), (0.1, 0), (0.1, 33), (0.1, 8, ()), (0.1, 8, ('objects',)), (0.1, 8, 7)):
        with pytest.raises(ValueError):
            g.rays(*args)


def test_batched_env_ray_obs():
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    from tests.objects_ref import object_sets
    E, N = 4, 64
    kw, centres = object_sets()['boxes']
    objs = np.tile(centres[None], (E, 1, 1))
    spawn = dict(seed=3, spawn_std=0.12, spawn_mean=(0.4, 0.3))        # (a cloud around the box at (0.5, 0.35))
    env = BatchedKilobotsEnv(E, N, ray_obs=(0.2, 12), **spawn, **kw)
    plain = BatchedKilobotsEnv(E, N, **spawn, **kw)
    assert env.ray_obs == (0.2, 12, 7)
    for e in (env, plain):
        e.sim.set_objects_m(objs)
    assert torch.equal(env.reset(), plain.reset())
    a = dev(scenes.random_actions(E, N, seed=20))
    obs, _, _, info = env.step(a)
    pobs, _, _, pinfo = plain.step(a)
    assert pinfo == {} and torch.equal(obs, pobs)
    assert sorted(info) == ['rays']
    dist, hit = env.sim.rays(0.2, 12)
    for got in (info['rays'], env.rays()):
        assert torch.equal(got[0].view(torch.int32), dist.view(torch.int32)) and torch.equal(got[1], hit)
    wd, wh = want(env.sim, 0.2, 12, 7)
    assert np.array_equal(bits(cpu(dist)), bits(wd)) and np.array_equal(cpu(hit), wh)
    assert (wh >= N + 4).any() and ((wh >= 0) & (wh < N)).any()
    with pytest.raises(ValueError):
        plain.rays()
    bare = BatchedKilobotsEnv(2, 16, seed=3, ray_obs=(0.3, 5, ('walls',)))
    bare.reset()
    info = bare.step(dev(scenes.random_actions(2, 16, seed=21)))[3]
    wd, wh = want(bare.sim, 0.3, 5, nat.RAY_WALLS)
    assert sorted(info) == ['rays'] and np.array_equal(bits(cpu(info['rays'][0])), bits(wd)) and np.array_equal(cpu(info['rays'][1]), wh)
