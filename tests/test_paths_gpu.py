"""kb_sense_paths on the GPU against the restatement of its definition (tests/paths_ref.py): Dijkstra's algorithm on Python
ints, which shares nothing with the kernel's sweeps, and the fixture walk in float32 on the outline of kb_get_outline.
Everything is compared for equality of the bit patterns, in every output: the distances are integers and every fp32
operation of the definition is rounded on its own, on the device and in the restatement.  No tolerances.  The constructed
scenes are those that tests/test_paths_cpu.py holds to what they are there for."""
import itertools

import numpy as np
import pytest
import torch

from tests import geometry_scenes as GS
from tests import objects_ref
from tests import paths_ref as ref
from tests.gpu_common import cpu, dev, object_state
from tests.paths_ref import random_masks, scattered
from tests.sensing_common import make_sim

pytestmark = pytest.mark.gpu

PARTS = ref.PARTS
KILOBOT_RADIUS = 0.0165
SETS = objects_ref.object_sets()


def want(g, gw, gh, source, blocked=None, objects=0, clear=0.0):
    """The restatement on the state of the sim as it is on the device; source, blocked: numpy masks [E, gh, gw]."""
    return ref.restate(objects_ref.tables(g.outline()), gw, gh, source, blocked, objects, clear, *object_state(g))[0]


def differing(t, w):
    a, b = cpu(t), np.asarray(w)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return a.view(np.uint32) != b.view(np.uint32) if a.dtype == np.float32 else a != b


def check(g, gw, gh, source, blocked=None, objects=0, clear=0.0, what='', w=None):
    w = want(g, gw, gh, source, blocked, objects, clear) if w is None else w
    got = g.paths(gw, gh, dev(source), None if blocked is None else dev(blocked), objects=objects, clearance_m=clear)
    torch.cuda.synchronize()
    assert got._fields == PARTS and got.step.dtype == torch.int8 and got.dist.dtype == got.bots.dtype == got.stats.dtype == torch.float32
    for name in PARTS:
        d = differing(getattr(got, name), getattr(w, name))
        print('%s E=%d N=%d %d x %d objects %d clear %g %s: %d of %d differ' % (what, g.num_envs, g.num_bots, gw, gh, objects, clear, name, int(d.sum()), d.size))
        assert not d.any(), (what, gw, gh, name, np.argwhere(d)[:5])
    return w


# 1 x 1; a single row and a single column; odd, non-square cells; the serpentine, whose sweep count is far beyond gw + gh;
# several cells per lane; the largest grid, where the LDS image is at its limit and a lane holds the most cells
@pytest.mark.parametrize('gw,gh,E,N', [(1, 1, 5, 1), (1, 7, 2, 7), (5, 1, 2, 7), (7, 5, 3, 333), (33, 31, 2, 7), (64, 48, 2, 1024), (128, 128, 2, 333)])
def test_grids_equal_the_restatement(gw, gh, E, N):
    """Env 0 carries the serpentine with the source at one end of the corridor, the others random walls and sources; the last
    env of a batch of three or more has no source at all."""
    xy, th = scattered(E, N, seed=gw * gh + N)
    g = make_sim(E, N, xy, th)
    source, blocked = random_masks(E, gw, gh, seed=gw + gh)
    blocked[0], source[0] = ref.serpentine(gw, gh), ref.mask_of(gw, gh, [(0, 0)])
    if E >= 3:
        source[E - 1] = 0
    w = check(g, gw, gh, source, blocked, what='grids')
    assert np.isfinite(w.dist[0][blocked[0] == 0]).all() and w.stats[0, 3] == (blocked[0] == 0).sum()
    if E >= 3:
        assert np.isposinf(w.dist[E - 1]).all() and (w.bots[E - 1, :, 3] == 3).all() and not w.stats[E - 1].any()
        assert (w.step[E - 1][blocked[E - 1] == 0] == -2).all() and (w.step[E - 1][blocked[E - 1] != 0] == -3).all()
    if (gw, gh) != (128, 128):
        check(g, gw, gh, source, None, what='no walls')


def test_constructed_scenes():
    """One batch on the 7 x 5 grid with the kilobots of the mixed scene in every env: the mixed scene (every flag, a blocked
    source, tied directions, kilobots outside the arena and on blocked cells with and without a way out), two obstacles
    touching at a corner, every cell blocked, no source, and a source region of many cells."""
    gw, gh, src0, blk0, xy, th = ref.mixed_scene()
    E = 5
    g = make_sim(E, len(xy), np.tile(xy, (E, 1, 1)), np.tile(th, (E, 1)))
    source, blocked = np.zeros((E, gh, gw), dtype=np.uint8), np.zeros((E, gh, gw), dtype=np.uint8)
    source[0], blocked[0] = src0, blk0
    source[1], blocked[1] = ref.mask_of(gw, gh, [(0, 0)]), ref.corner_scene(gw, gh)
    source[2], blocked[2] = 1, 1
    blocked[3] = blk0
    source[4, 1:4, 2:6] = 1
    w = check(g, gw, gh, source, blocked, what='constructed')
    assert w.bots[0, :, 3].tolist() == [1, 0, 2, 3, 3, 0, 3]
    assert (w.step[2] == -3).all() and (w.bots[2, :, 3] == 3).all() and not w.stats[2].any()
    assert np.isposinf(w.dist[3]).all() and not w.stats[3].any() and (w.bots[3, :, 3] == 3).all()
    assert w.stats[4, 3] == gw * gh and (w.dist[4, 1:4, 2:6] == 0).all() and (w.step[4, 1:4, 2:6] == -1).all()
    # the same masks as bool tensors
    got = g.paths(gw, gh, dev(source).ne(0), dev(blocked).ne(0))
    for name in PARTS:
        assert not differing(getattr(got, name), getattr(w, name)).any(), name


def make_objects(E, N, name, seed):
    kw, centres = SETS[name]
    xy, th, objs, oth = objects_ref.spawn_over_objects(E, N, centres, seed)
    g = make_sim(E, N, xy, th, **kw)
    g.set_objects_m(objs, oth)
    return g


@pytest.mark.parametrize('clear', [0.0, KILOBOT_RADIUS])
@pytest.mark.parametrize('name', ['disc', 'boxes', 'forms'])
def test_objects_block(name, clear):
    """A disc, four rotated boxes and the LForm / TForm / CForm scene, the kilobots drawn around the objects so that some stand
    on blocked cells: all objects, a strict subset and none; objects alone, d_blocked alone and both."""
    E, N = 2, 64
    g = make_objects(E, N, name, seed=7)
    M = g.num_objects
    subset = 1 if M == 1 else (1 << M) - 2
    for gw, gh in ((64, 48), (7, 5)):
        source, blocked = random_masks(E, gw, gh, seed=M, density=0.1)
        every = check(g, gw, gh, source, None, (1 << M) - 1, clear, what=name)
        both = check(g, gw, gh, source, blocked, (1 << M) - 1, clear, what=name + ' + d_blocked')
        check(g, gw, gh, source, None, subset, clear, what=name + ' subset')
        walls = check(g, gw, gh, source, blocked, 0, clear, what=name + ' d_blocked alone')
        if (gw, gh) == (64, 48):
            assert (every.bots[..., 3] == 2).any() and np.isinf(every.dist).sum() < np.isinf(both.dist).sum() > np.isinf(walls.dist).sum()
    # 'all' and an iterable of indices are the masks
    source = dev(random_masks(E, 64, 48, seed=M)[0])
    a, b = g.paths(64, 48, source, clearance_m=clear), g.paths(64, 48, source, objects=range(M), clearance_m=clear)
    for name_ in PARTS:
        assert torch.equal(getattr(a, name_).view(torch.uint8), getattr(b, name_).view(torch.uint8))


def test_an_arena_off_the_default():
    row = next(r for r in GS.GEOMETRY if r.name == '3.6x2.7-200-sleep')
    s = GS.scene(row)
    g = make_sim(s.E, s.N, s.xy, s.th, **s.kw)
    assert g.outline().arena[1] == np.float32(0.5) * (np.float32(row.W) * np.float32(25.0))
    for gw, gh in ((7, 5), (64, 48)):
        source, blocked = random_masks(s.E, gw, gh, seed=5)
        w = check(g, gw, gh, source, blocked, what=row.name)
        assert np.isfinite(w.stats).all() and w.stats[:, 0].any()
        assert g.path_costs(gw, gh) == ref.costs(objects_ref.tables(g.outline()), gw, gh)[0]


def test_every_subset_of_the_outputs_returns_the_same_words():
    """out= full of garbage comes back as the restatement with every non-empty subset of the outputs; the same tensors are
    returned, twice the same."""
    E, N = 3, 7
    g = make_objects(E, N, 'boxes', seed=9)
    for gw, gh in ((7, 5), (64, 48)):
        source, blocked = random_masks(E, gw, gh, seed=2, density=0.15)
        source[1] = 0
        w = want(g, gw, gh, source, blocked, 15, KILOBOT_RADIUS)
        shapes = {'dist': ((E, gh, gw), torch.float32), 'step': ((E, gh, gw), torch.int8), 'bots': ((E, N, 4), torch.float32), 'stats': ((E, 4), torch.float32)}
        ds, db = dev(source), dev(blocked)
        for k in range(1, 5):
            for names in itertools.combinations(PARTS, k):
                out = tuple(torch.full(shapes[n][0], 0x5B, dtype=torch.uint8, device='cuda').to(torch.int8) if n == 'step' else
                            torch.full(shapes[n][0], 0x7FC12345, dtype=torch.int32, device='cuda').view(torch.float32) for n in names)
                for _ in range(2):
                    got = g.paths(gw, gh, ds, db, clearance_m=KILOBOT_RADIUS, out=out, **{n: n in names for n in PARTS})
                    torch.cuda.synchronize()
                    for n in PARTS:
                        assert (getattr(got, n) is None) == (n not in names)
                    for n, o in zip(names, out):
                        assert getattr(got, n).data_ptr() == o.data_ptr()
                        assert not differing(o, getattr(w, n)).any(), (gw, gh, names, n)
    src = dev(source)
    with pytest.raises(ValueError):
        g.paths(64, 48, src, dist=False, step=False, bots=False, stats=False)
    off = torch.zeros(E * N * 4 + 1, device='cuda')[1:].view(E, N, 4)
    assert off.data_ptr() % 16 != 0
    with pytest.raises(ValueError):
        g.paths(64, 48, src, dist=False, step=False, stats=False, out=off)
    for bad in (src.float(), src[:, :-1].contiguous(), src.cpu(), None):
        with pytest.raises(ValueError):
            g.paths(64, 48, bad)
    for kw in (dict(objects=16), dict(objects='some'), dict(clearance_m=-1.0), dict(clearance_m=float('nan')), dict(blocked=src.float()),
               dict(out=torch.zeros(E, 48, 64, device='cuda'))):
        with pytest.raises(ValueError):
            g.paths(64, 48, src, **kw)
    for bad in ((0, 48), (64, 129)):
        with pytest.raises(ValueError):
            g.paths(*bad, src)


def test_rows_do_not_depend_on_the_other_envs():
    """Row e of a batch equals a one-env handle given env e's state."""
    E, N, gw, gh = 3, 64, 64, 48
    kw, centres = SETS['boxes']
    xy, th, objs, oth = objects_ref.spawn_over_objects(E, N, centres, seed=13)
    g = make_sim(E, N, xy, th, **kw)
    g.set_objects_m(objs, oth)
    source, blocked = random_masks(E, gw, gh, seed=4, density=0.1)
    full = g.paths(gw, gh, dev(source), dev(blocked), clearance_m=KILOBOT_RADIUS)
    for e in range(E):
        g1 = make_sim(1, N, xy[e:e + 1], th[e:e + 1], **kw)
        g1.set_objects_m(objs[e:e + 1], oth[e:e + 1])
        one = g1.paths(gw, gh, dev(source[e:e + 1]), dev(blocked[e:e + 1]), clearance_m=KILOBOT_RADIUS)
        torch.cuda.synchronize()
        for name in PARTS:
            assert torch.equal(getattr(one, name).view(torch.uint8), getattr(full, name)[e:e + 1].contiguous().view(torch.uint8)), (e, name)


def test_path_cells_on_the_device_is_the_host_rule():
    from gym_kilobots_amd import _native as nat
    g = make_sim(2, 7)
    pts = np.array([[0.0, 0.0], [-1.0, -0.75], [0.99, 0.74], [2.0, 0.1]], dtype=np.float32)
    shared = g.path_cells(pts, 7, 5)
    assert shared.dtype == torch.uint8 and tuple(shared.shape) == (2, 5, 7) and shared.is_cuda
    assert np.array_equal(cpu(shared), np.tile(nat.path_cells(g.outline().arena, pts, 7, 5), (2, 1, 1)))
    per_env = g.path_cells(torch.from_numpy(np.stack([pts[:2], pts[2:]])).cuda(), 7, 5)
    assert np.array_equal(cpu(per_env), nat.path_cells(g.outline().arena, np.stack([pts[:2], pts[2:]]), 7, 5))
    with pytest.raises(ValueError):
        g.path_cells(np.zeros((3, 4, 2), dtype=np.float32), 7, 5)


def test_batched_env_path_obs():
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    from tests import scenes
    E, N = 2, 64
    kw, centres = SETS['boxes']
    init = np.concatenate([centres, np.array([[0.3], [0.7], [1.1], [1.9]])], 1)
    env = BatchedKilobotsEnv(E, N, seed=3, path_obs=(32, 24, KILOBOT_RADIUS), object_init=init, **kw)
    plain = BatchedKilobotsEnv(E, N, seed=3, object_init=init, **kw)
    assert torch.equal(env.reset(), plain.reset())
    a = dev(scenes.random_actions(E, N, seed=20))
    first = env.paths()
    assert (cpu(first.bots)[..., 3] == 3).all() and not cpu(first.stats).any()        # no goal yet
    goal = np.array([[0.8, 0.6], [-0.9, -0.7]])
    env.set_path_goal(points_m=goal)
    walls = np.zeros((24, 32), dtype=np.uint8)
    walls[5:20, 16] = 1
    env.set_path_blocked(walls)
    obs, _, _, info = env.step(a)
    pobs, _, _, pinfo = plain.step(a)
    assert pinfo == {} and torch.equal(obs, pobs)
    assert sorted(info) == ['paths'] and info['paths']._fields == PARTS
    source = cpu(env.sim.path_cells(goal, 32, 24))
    blocked = np.tile(walls, (E, 1, 1))
    direct = env.sim.paths(32, 24, dev(source), dev(blocked), clearance_m=KILOBOT_RADIUS)
    w = want(env.sim, 32, 24, source, blocked, 15, KILOBOT_RADIUS)
    for name in PARTS:
        for got in (info['paths'], direct, env.paths()):
            assert not differing(getattr(got, name), getattr(w, name)).any(), name
    assert w.stats[:, 0].all() and source.sum() == 2 * E
    env.set_path_goal(cells=source[0])
    env.set_path_blocked(None)
    w = want(env.sim, 32, 24, np.tile(source[0], (E, 1, 1)), None, 15, KILOBOT_RADIUS)
    for name in PARTS:
        assert not differing(getattr(env.paths(), name), getattr(w, name)).any(), name
    with pytest.raises(ValueError):
        plain.paths()
