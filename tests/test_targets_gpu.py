"""kb_sense_targets on the GPU against the numpy restatement of its definition (tests/targets_ref.py), a brute force over the
full [N, K] matrix that shares nothing with the kernel.  Everything is compared for equality of the bit patterns: every
operation of the definition is one fp32 operation rounded on its own, the sums are integers, on the device and in the
restatement.  No tolerances.  The scenes are those of tests/targets_scenes.py, which tests/test_targets_cpu.py holds to what
they are there for."""
import numpy as np
import pytest
import torch

from tests import targets_scenes as TS
from tests.gpu_common import cpu, dev
from tests.sensing_checks import TARGETS_PARTS as PARTS, check_targets as check, differing, want_targets as want
from tests.sensing_common import make_sim

pytestmark = pytest.mark.gpu


def sim_of(sc):
    """(sim holding the scene's poses, the keyword arguments of targets() on the device)"""
    g = make_sim(*sc.x.shape)
    g.x.copy_(dev(sc.x))
    g.y.copy_(dev(sc.y))
    g.theta.copy_(dev(sc.th))
    return g, dict(bot_select=None if sc.bsel is None else dev(sc.bsel), slot_select=None if sc.ssel is None else dev(sc.ssel))


@pytest.mark.parametrize('name', sorted(TS.SCENES))
def test_scene_equals_the_restatement(name):
    sc = TS.SCENES[name]()
    g, sel = sim_of(sc)
    w = check(g, dev(sc.points), sc.tol, what=name, **sel)
    if name == 'ties':
        assert (w.owner[0, 2], w.index[0, 0], w.owner[1, 3], w.index[1, 6]) == (1, 0, 3, 2)
    if name == 'contested':
        assert w.rel[0, :, 3].tolist() == [1.0, 0.0, 1.0]
    if name == 'tolerance':
        assert w.stats[0, 4:].tolist() == [2.0, 2.0]
        zero = check(g, dev(sc.points), 0.0, what='tolerance 0', **sel)
        assert zero.stats[0, 4:].tolist() == [1.0, 1.0]
    if name == 'masks':
        assert np.isposinf(w.stats[2:, :4]).all() and (w.index[2:] == -1).all() and (w.owner[2:] == -1).all()


def test_bool_and_uint8_masks():
    sc = TS.masks()
    g, sel = sim_of(sc)
    points = dev(sc.points)
    w = want(g, points, sc.tol, **sel)
    as_bool = {k: v.ne(0) for k, v in sel.items()}
    assert all(v.dtype == torch.bool for v in as_bool.values())
    check(g, points, sc.tol, what='bool masks', w=w, alone=False, **as_bool)
    # one side masked at a time, and a selection of ones is everyone
    check(g, points, sc.tol, what='kilobots masked', bot_select=sel['bot_select'])
    check(g, points, sc.tol, what='slots masked', slot_select=sel['slot_select'])
    everyone = check(g, points, sc.tol, what='everyone', alone=False)
    check(g, points, sc.tol, what='all selected', w=everyone, alone=False, **{k: torch.ones_like(v) for k, v in sel.items()})


def test_shared_points_equal_per_env_points():
    sc = TS.shared()
    g, sel = sim_of(sc)
    points = dev(sc.points)
    assert points.dim() == 2
    w = check(g, points, sc.tol, what='shared')
    check(g, points[None].expand(3, -1, -1).contiguous(), sc.tol, what='per env', w=w)
    mask = dev((np.random.RandomState(70).rand(3, 40) < 0.5).astype(np.uint8))      # (the slot mask is per env also with shared points)
    w = check(g, points, sc.tol, what='shared, masked', slot_select=mask)
    assert (w.owner[0] != w.owner[1]).any() and ((w.owner == -1) == (cpu(mask) == 0)).all()


def test_rows_do_not_depend_on_the_other_envs():
    """Row e of a batch equals a one-env handle given env e's poses, points and masks."""
    sc = TS.masks()
    g, sel = sim_of(sc)
    full = g.targets(dev(sc.points), sc.tol, **sel)
    for e in range(sc.x.shape[0]):
        one = TS.Scene(sc.x[e:e + 1], sc.y[e:e + 1], sc.th[e:e + 1], sc.points[e:e + 1], sc.tol, sc.bsel[e:e + 1], sc.ssel[e:e + 1])
        g1, s1 = sim_of(one)
        got = g1.targets(dev(one.points), sc.tol, **s1)
        torch.cuda.synchronize()
        for name in PARTS:
            assert torch.equal(getattr(got, name).view(torch.int32), getattr(full, name)[e:e + 1].view(torch.int32)), (e, name)


def test_every_element_is_written():
    """out= full of garbage comes back as the restatement, with all outputs and with each subset that leaves one out, on a
    scene with unselected entries and empty envs; the same tensors are returned, twice the same."""
    sc = TS.masks()
    g, sel = sim_of(sc)
    points = dev(sc.points)
    E, N = sc.x.shape
    K = sc.points.shape[-2]
    w = want(g, points, sc.tol, **sel)
    shapes = {'index': ((E, N), torch.int32), 'rel': ((E, N, 4), torch.float32), 'owner': ((E, K), torch.int32), 'dist': ((E, K), torch.float32),
              'stats': ((E, 6), torch.float32)}
    for left_out in (None,) + PARTS:
        names = [n for n in PARTS if n != left_out]
        out = tuple(torch.full(shapes[n][0], 0x7FC12345, dtype=torch.int32, device='cuda').view(shapes[n][1]) for n in names)
        for _ in range(2):
            got = g.targets(points, sc.tol, out=out, **sel, **{n: n != left_out for n in PARTS})
            torch.cuda.synchronize()
            for n, o in zip(names, out):
                assert getattr(got, n).data_ptr() == o.data_ptr()
                assert not differing(o, getattr(w, n)).any(), (left_out, n)


def test_bad_tensors_raise():
    sc = TS.shared()
    g, sel = sim_of(sc)
    points = dev(sc.points)
    E, N, K = 3, 50, 40
    for bad in (points.double(), points.cpu(), points.t(), points[:, :1].contiguous(), points[None].expand(2, -1, -1).contiguous(), cpu(points),
                torch.zeros(0, 2, device='cuda'), torch.zeros(1025, 2, device='cuda'), points.flatten()):
        with pytest.raises(ValueError):
            g.targets(bad, sc.tol)
    for tol in (-0.01, float('inf'), float('nan')):
        with pytest.raises(ValueError):
            g.targets(points, tol)
    mask = torch.ones(E, N, dtype=torch.uint8, device='cuda')
    for bad in (mask.float(), mask[:, :-1].contiguous(), mask.cpu(), mask.t(), torch.ones(E, K, dtype=torch.uint8, device='cuda')):
        with pytest.raises(ValueError):
            g.targets(points, sc.tol, bot_select=bad)
    for bad in (torch.ones(K, dtype=torch.uint8, device='cuda'), mask, torch.ones(E, K, device='cuda')):
        with pytest.raises(ValueError):
            g.targets(points, sc.tol, slot_select=bad)
    with pytest.raises(ValueError):
        g.targets(points, sc.tol, index=False, rel=False, owner=False, dist=False, stats=False)
    bad_outs = [torch.zeros(E, N, dtype=torch.int32, device='cuda'),
                (torch.zeros(E, N, dtype=torch.int32, device='cuda'),) * 5,
                (torch.zeros(E, N, dtype=torch.int32, device='cuda'), torch.zeros(E, N, 4, device='cuda'), torch.zeros(E, K, dtype=torch.int32, device='cuda'),
                 torch.zeros(E, K, device='cuda'), torch.zeros(E, 2, device='cuda'))]
    for bad in bad_outs:
        with pytest.raises(ValueError):
            g.targets(points, sc.tol, out=bad)
    off = torch.zeros(E * N * 4 + 1, device='cuda')[1:].view(E, N, 4)
    assert off.data_ptr() % 16 != 0
    with pytest.raises(ValueError):
        g.targets(points, sc.tol, index=False, owner=False, dist=False, stats=False, out=off)


def test_batched_env_target_obs():
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    from tests import scenes
    E, N, K = 2, 64, 24
    pts = np.random.RandomState(71).uniform(-0.3, 0.3, size=(K, 2))
    env = BatchedKilobotsEnv(E, N, seed=3, target_obs=(pts, 0.03))
    plain = BatchedKilobotsEnv(E, N, seed=3)
    assert torch.equal(env.reset(), plain.reset())
    a = dev(scenes.random_actions(E, N, seed=20))
    obs, _, _, info = env.step(a)
    pobs, _, _, pinfo = plain.step(a)
    assert pinfo == {} and torch.equal(obs, pobs)
    assert sorted(info) == ['targets'] and info['targets']._fields == PARTS
    points = dev(pts.astype(np.float32))
    direct = env.sim.targets(points, 0.03)
    again = env.targets()
    w = want(env.sim, points, 0.03)
    for name in PARTS:
        for got in (info['targets'], direct, again):
            assert not differing(getattr(got, name), getattr(w, name)).any(), name
    assert tuple(info['targets'].index.shape) == (E, N) and tuple(info['targets'].dist.shape) == (E, K)
    # the slot mask and new points: what the next observation is taken over
    mask = dev((np.random.RandomState(72).rand(E, K) < 0.5).astype(np.uint8))
    env.set_targets(slot_select=mask)
    w = want(env.sim, points, 0.03, slot_select=mask)
    assert not any(differing(getattr(env.targets(), n), getattr(w, n)).any() for n in PARTS)
    per_env = np.random.RandomState(73).uniform(-0.3, 0.3, size=(E, K, 2)).astype(np.float32)
    env.set_targets(per_env)
    w = want(env.sim, dev(per_env), 0.03)
    assert not any(differing(getattr(env.targets(), n), getattr(w, n)).any() for n in PARTS)
    with pytest.raises(ValueError):
        env.set_targets(per_env[:, :-1])
    with pytest.raises(ValueError):
        plain.targets()
