"""kb_sense_coverage on the GPU against the numpy restatement of its definition (tests/coverage_ref.py), a brute force over
all candidates that shares nothing with the kernel's search.  Everything is compared for equality of the bit patterns:
every operation of the definition is one fp32 operation rounded on its own, the accumulators are integers, on the device
and in the restatement.  No tolerances.  The scenes are those of tests/coverage_scenes.py, which tests/test_coverage_cpu.py
holds to what they are there for."""
import numpy as np
import pytest
import torch

from tests import coverage_scenes as CS
from tests.gpu_common import dev
from tests.sensing_checks import COVERAGE_PARTS as PARTS, check_coverage as check, differing, want_coverage as want
from tests.sensing_common import make_sim

pytestmark = pytest.mark.gpu

GRIDS = [(1, 1), (3, 2), (7, 5), (64, 48), (127, 95), (128, 128)]


def sim_of(scene, **kw):
    """(sim holding the scene's poses, select on the device or None, the scene)"""
    x, y, th, sel = scene
    g = make_sim(x.shape[0], x.shape[1], **kw)
    g.x.copy_(dev(x))
    g.y.copy_(dev(y))
    g.theta.copy_(dev(th))
    return g, None if sel is None else dev(sel)


def test_ties_go_to_the_lower_index():
    """Seven kilobots are worth one ring, which settles nothing: these ties are those of the scan of all kilobots."""
    g, sel = sim_of(CS.ties())
    w = check(g, *CS.TIE_GRID, what='ties')
    assert (w.owner[0, 36, 24], w.owner[1, 36, 24]) == (0, 3)
    for gw, gh in ((7, 5), (128, 128)):         # the same kilobots on grids whose constants are rounded
        check(g, gw, gh, what='ties')


def test_ring_ties_go_to_the_lower_index():
    """Ties that the RING search settles (128 kilobots are worth four rings): the tied kilobots lie in different rings around
    the centre, and in env 0 the lower index lies in the outer one, so that a search which stopped a ring early or took ties
    in the order of the chains would name another owner (tests/test_coverage_cpu.py holds the scene to that)."""
    g, sel = sim_of(CS.ring_ties())
    w = check(g, *CS.TIE_GRID, what='ring ties')
    (cx, cy), d, _, _ = CS.RING_TIES[2]         # the pair in rings 2 | 3 around (14.5, -11.5): cell (39, 14) of the grid
    assert (w.owner[0, 14, 39], w.owner[1, 14, 39]) == (2, 128 - 1 - 6) and w.dist[0, 14, 39] == np.float32(d) / np.float32(25.0)
    for gw, gh in ((64, 48), (128, 128)):
        check(g, gw, gh, what='ring ties', alone=False)


def test_all_kilobots_in_a_far_corner():
    """15 x 11 broadphase cells of 3.5 and 1024 kilobots in one corner cell: most centres find nothing until the ring that holds
    the far corner of the grid and end their search on it, the rest lie beyond the eleven rings and scan."""
    g, sel = sim_of(CS.far_corner(), **CS.FAR_CORNER_KW)
    for gw, gh in ((64, 48), (7, 5)):
        w = check(g, gw, gh, what='far corner', alone=False)
        assert (w.owner >= 0).all()


def test_one_kilobot():
    """One kilobot in a corner of the arena, and outside it.  The budget gives one kilobot no ring at all, so this is the scan
    of all kilobots, not a ring search across the grid (that is test_all_kilobots_in_a_far_corner)."""
    g, sel = sim_of(CS.one())
    for gw, gh in ((64, 48), (1, 1), (128, 128)):
        w = check(g, gw, gh, what='one')
        assert not w.owner.any() and (w.cells[:, 0, 2] == gw * gh).all()


@pytest.mark.parametrize('gw,gh', GRIDS)
def test_walls(gw, gh):
    g, sel = sim_of(CS.walls())
    check(g, gw, gh, what='walls')


@pytest.mark.parametrize('gw,gh', CS.DENSE_GRIDS)
def test_dense(gw, gh):
    g, sel = sim_of(CS.dense())
    check(g, gw, gh, what='dense')


def test_select():
    x, y, th, sel_h = CS.select()
    g, sel = sim_of((x, y, th, sel_h))
    w = check(g, 64, 48, sel, what='select')
    assert (w.owner[2] == -1).all() and (w.owner[1] == 217).all() and np.isposinf(w.stats[2]).all()
    check(g, 64, 48, sel.ne(0), what='select as bool', w=w)
    assert sel.ne(0).dtype == torch.bool
    check(g, 7, 5, sel, what='select')
    # None is everyone, and so is a selection of ones
    everyone = check(g, 64, 48, None, what='everyone')
    check(g, 64, 48, torch.ones_like(sel), what='all selected', w=everyone, alone=False)
    for bad in (sel.float(), sel[:, :-1].contiguous(), sel.cpu(), sel.t()):
        with pytest.raises(ValueError):
            g.coverage(64, 48, select=bad)
    with pytest.raises(ValueError):
        g.coverage(64, 48, owner=False, dist=False, cells=False, stats=False)
    for bad in ((0, 48), (64, 129)):
        with pytest.raises(ValueError):
            g.coverage(*bad)


def test_rows_do_not_depend_on_the_other_envs():
    """Row e of a batch equals a one-env handle given env e's poses."""
    x, y, th, sel_h = CS.select()
    g, sel = sim_of((x, y, th, sel_h))
    full = g.coverage(64, 48, select=sel)
    for e in range(x.shape[0]):
        g1, s1 = sim_of((x[e:e + 1], y[e:e + 1], th[e:e + 1], sel_h[e:e + 1]))
        one = g1.coverage(64, 48, select=s1)
        torch.cuda.synchronize()
        for name in PARTS:
            assert torch.equal(getattr(one, name).view(torch.int32), getattr(full, name)[e:e + 1].view(torch.int32)), (e, name)


def test_every_element_is_written():
    """out= full of garbage comes back as the restatement, with all outputs, with each subset that leaves one out, and with
    an env that has no candidate; the same tensors are returned, twice the same."""
    x, y, th, sel_h = CS.select()
    g, sel = sim_of((x, y, th, sel_h))
    E, N = x.shape
    for gw, gh in ((64, 48), (7, 5), (127, 95)):
        w = want(g, gw, gh, sel)
        shapes = {'owner': ((E, gh, gw), torch.int32), 'dist': ((E, gh, gw), torch.float32), 'cells': ((E, N, 4), torch.float32), 'stats': ((E, 2), torch.float32)}
        for left_out in (None,) + PARTS:
            names = [n for n in PARTS if n != left_out]
            out = tuple(torch.full(shapes[n][0], 0x7FC12345, dtype=torch.int32, device='cuda').view(shapes[n][1]) for n in names)
            for _ in range(2):
                got = g.coverage(gw, gh, select=sel, out=out, **{n: n != left_out for n in PARTS})
                torch.cuda.synchronize()
                for n, o in zip(names, out):
                    assert getattr(got, n).data_ptr() == o.data_ptr()
                    assert not differing(o, getattr(w, n)).any(), (gw, gh, left_out, n)
    bad_outs = [torch.zeros(E, 48, 64, dtype=torch.int32, device='cuda'),
                (torch.zeros(E, 48, 64, dtype=torch.float32, device='cuda'),) * 4,
                (torch.zeros(E, 48, 64, dtype=torch.int32, device='cuda'), torch.zeros(E, 64, 48, device='cuda'), torch.zeros(E, N, 4, device='cuda'), torch.zeros(E, 2, device='cuda'))]
    for bad in bad_outs:
        with pytest.raises(ValueError):
            g.coverage(64, 48, out=bad)
    off = torch.zeros(E * N * 4 + 1, device='cuda')[1:].view(E, N, 4)
    assert off.data_ptr() % 16 != 0
    with pytest.raises(ValueError):
        g.coverage(64, 48, owner=False, dist=False, stats=False, out=off)


def test_batched_env_coverage_obs():
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    from tests import scenes
    E, N = 2, 64
    env = BatchedKilobotsEnv(E, N, seed=3, coverage_obs=(32, 24))
    plain = BatchedKilobotsEnv(E, N, seed=3)
    assert torch.equal(env.reset(), plain.reset())
    a = dev(scenes.random_actions(E, N, seed=20))
    obs, _, _, info = env.step(a)
    pobs, _, _, pinfo = plain.step(a)
    assert pinfo == {} and torch.equal(obs, pobs)
    assert sorted(info) == ['coverage'] and info['coverage']._fields == PARTS
    direct = env.sim.coverage(32, 24)
    again = env.coverage()
    w = want(env.sim, 32, 24)
    for name in PARTS:
        for got in (info['coverage'], direct, again):
            assert not differing(getattr(got, name), getattr(w, name)).any(), name
    assert tuple(info['coverage'].owner.shape) == (E, 24, 32) and tuple(info['coverage'].cells.shape) == (E, N, 4)
    with pytest.raises(ValueError):
        plain.coverage()
