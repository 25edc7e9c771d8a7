"""kb_sense_neighbors on the GPU against a brute-force numpy restatement of its definition (include/kilobots_hip.h).

The restatement works on float32 arrays only, so every operation rounds on its own like the kernel's (-ffp-contract=off):
all pairs of an env, the predicate !(d2 > R2), np.lexsort by (d2, j), the oracle's sincosf for the frame.  Everything is
compared for equality: indices and counts as integers, rel by its bit patterns.  No tolerances."""
import numpy as np
import pytest
import torch

from tests import scenes
from tests.gpu_common import cpu, dev, state
from tests.sensing_checks import check_neighbors as check, restate_neighbors as restate
from tests.sensing_common import SWEEP, make_sim, sweep_scene, wall_scene

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('k', [1, 4, 8, 16])
@pytest.mark.parametrize('E,N,R', SWEEP)
def test_lists_equal_the_restatement(E, N, R, k):
    xy, th = sweep_scene(E, N)
    g = make_sim(E, N, xy, th)
    _, _, cnt, _ = check(g, R, k, 'sweep')
    assert cnt.max() > 0 or N == 1


@pytest.mark.parametrize('k', [1, 4, 8, 16])
@pytest.mark.parametrize('R', [0.04, 0.09, 0.15])
def test_lists_at_walls_and_corners(R, k):
    xy, th = wall_scene()
    g = make_sim(4, xy.shape[1], xy, th)
    x, y = state(g)[:2]
    assert (np.abs(x) > 25.0).any() and (np.abs(y) > 18.75).any()      # some kilobots are outside: their cell indices clamp
    check(g, R, k, 'walls')


@pytest.mark.parametrize('k', [4, 8, 16])
def test_coincident_kilobots_are_ordered_by_index(k):
    """std = 3 m clips most of the cloud onto the spawn bounds: piles of kilobots at exactly the same point in the corners
    and along the edges, d2 == 0 ties that only the index order resolves."""
    E, N, R = 4, 200, 0.07
    g = make_sim(E, N)
    g.reset(seed=7, std=3.0, resolve=False)
    idx, rel, cnt, zeros = check(g, R, k, 'coincident')
    assert zeros.max() > k, 'the seed must put more than k kilobots on one point'
    e, i = np.unravel_index(zeros.argmax(), zeros.shape)
    assert (rel[e, i, :, 2] == 0).all() and (np.diff(idx[e, i]) > 0).all()      # k zero-distance slots, ascending indices


def test_headings_and_untouched_state():
    """Non-zero headings on stepped poses; the call reads the state and writes its outputs only."""
    E, N, R, k = 4, 128, 0.07, 8
    g = make_sim(E, N)
    g.reset(seed=11, std=0.12, random_theta=True)
    for s in range(3):
        g.step(4, actions=dev(scenes.random_actions(E, N, seed=80 + s)))
    torch.cuda.synchronize()
    assert float(g.theta.abs().max()) > 1.0
    fields = ('x', 'y', 'theta', 'ws_cnt', 'ws_key', 'ws_acc', 'status')
    before = {f: getattr(g, f).clone() for f in fields}
    idx, rel, cnt, _ = check(g, R, k, 'stepped')
    assert (rel[..., 3] != 0).any() and (rel[..., 1] != 0).any()
    torch.cuda.synchronize()
    for f in fields:
        a, b = before[f], getattr(g, f)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f


def test_more_slots_than_neighbours():
    E, N = 2, 7
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.2, seed=4)
    g = make_sim(E, N, xy, th)
    idx, rel, cnt, _ = check(g, 0.5, 16, 'k > N - 1')
    assert cnt.max() <= N - 1 and (idx[:, :, N - 1:] == -1).all()


def test_a_single_kilobot_has_only_padding():
    g = make_sim(5, 1, *scenes.gaussian_spawn(5, 1, sigma=0.2, seed=4))
    for k in (1, 8):
        idx, rel, cnt, _ = check(g, 0.1, k, 'N = 1')
        assert (idx == -1).all() and not rel.any() and not cnt.any()


def test_preallocated_outputs_are_reused():
    E, N, R, k = 3, 100, 0.08, 8
    g = make_sim(E, N, *scenes.gaussian_spawn(E, N, sigma=0.15, seed=5))
    out = (torch.full((E, N, k), 77, dtype=torch.int32, device='cuda'), torch.full((E, N, k, 4), 7.0, device='cuda'),
           torch.full((E, N), 77, dtype=torch.int32, device='cuda'))
    ptrs = [t.data_ptr() for t in out]
    got = g.neighbors(R, k, out=out)
    assert [t.data_ptr() for t in got] == ptrs
    first = [cpu(t).copy() for t in got]
    widx, wrel, wcnt, _ = restate(*state(g), R, k)
    assert np.array_equal(first[0], widx) and np.array_equal(first[1].view(np.uint32), wrel.view(np.uint32))
    assert np.array_equal(first[2].view(np.uint32), wcnt)
    # move the swarm, call again into the same tensors: every slot is rewritten (stale entries would survive as garbage)
    xy2, th2 = scenes.gaussian_spawn(E, N, sigma=0.3, seed=6)
    g.set_poses_m(xy2, th2)
    got = g.neighbors(R, k, out=out)
    assert [t.data_ptr() for t in got] == ptrs
    widx, wrel, wcnt, _ = restate(*state(g), R, k)
    assert np.array_equal(cpu(got[0]), widx) and np.array_equal(cpu(got[1]).view(np.uint32), wrel.view(np.uint32))
    assert np.array_equal(cpu(got[2]).view(np.uint32), wcnt)
    assert not np.array_equal(first[0], widx)
    # count=False: two tensors, no count written
    idx2, rel2, none = g.neighbors(R, k, out=out[:2], count=False)
    assert none is None and np.array_equal(cpu(idx2), widx)
    for bad in ((out[0], out[1]), (out[0].view(E, N * k), out[1], out[2]), (out[0].float(), out[1], out[2]), (out[0], out[1].cpu(), out[2]),
                (out[0], out[1][..., :2], out[2])):
        with pytest.raises(ValueError):
            g.neighbors(R, k, out=bad)
    with pytest.raises(ValueError):
        g.neighbors(R, 17)


def test_on_a_side_stream():
    E, N, R, k = 4, 256, 0.07, 8
    g = make_sim(E, N, *scenes.gaussian_spawn(E, N, sigma=0.2, seed=8))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        idx, rel, cnt = g.neighbors(R, k)
    side.synchronize()
    widx, wrel, wcnt, _ = restate(*state(g), R, k)
    assert np.array_equal(cpu(idx), widx) and np.array_equal(cpu(rel).view(np.uint32), wrel.view(np.uint32))
    assert np.array_equal(cpu(cnt).view(np.uint32), wcnt)


def test_a_shard_equals_its_rows():
    E, N, R, k, a, b = 6, 200, 0.07, 8, 2, 5
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.2, seed=12)
    g = make_sim(E, N, xy, th)
    part = make_sim(b - a, N, xy[a:b], th[a:b])
    whole, shard = g.neighbors(R, k), part.neighbors(R, k)
    for w, s in zip(whole, shard):
        assert torch.equal(w[a:b].contiguous().view(torch.uint8), s.view(torch.uint8))
    assert int(whole[2].max()) > 0


def test_batched_env_neighbor_obs():
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    E, N = 5, 80
    env = BatchedKilobotsEnv(E, N, seed=3, spawn_std=0.12, neighbor_obs=(0.07, 8))
    plain = BatchedKilobotsEnv(E, N, seed=3, spawn_std=0.12)
    assert torch.equal(env.reset(), plain.reset())
    for s in range(2):
        a = dev(scenes.random_actions(E, N, seed=20 + s))
        obs, rew, done, info = env.step(a)
        obs_p, _, _, info_p = plain.step(a)
        assert info_p == {} and set(info) == {'neighbors'}
        assert torch.equal(obs, obs_p)
        want = env.sim.neighbors(0.07, 8)
        for got, w in zip(info['neighbors'], want):
            assert torch.equal(got, w)
        for got, w in zip(env.neighbors(), want):
            assert torch.equal(got, w)
    idx, rel, cnt = (cpu(t) for t in info['neighbors'])
    widx, wrel, wcnt, _ = restate(*state(env.sim), 0.07, 8)
    assert np.array_equal(idx, widx) and np.array_equal(rel.view(np.uint32), wrel.view(np.uint32)) and np.array_equal(cnt.view(np.uint32), wcnt)
    assert int(wcnt.max()) > 0
    with pytest.raises(ValueError):
        plain.neighbors()
    with pytest.raises(ValueError):
        BatchedKilobotsEnv(E, N, neighbor_obs=(0.07, 17))
