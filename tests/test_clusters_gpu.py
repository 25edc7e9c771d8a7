"""kb_sense_clusters on the GPU against the brute-force numpy restatement of its definition (tests/clusters_ref.py).

Labels, sizes and stats are integers, the table is compared by its bit patterns: everything for equality, no tolerances."""
import itertools

import numpy as np
import pytest
import torch

from tests import clusters_ref as ref
from tests import scenes
from tests.gpu_common import Spy, cpu, dev, ranges, state
from tests.sensing_checks import CLUSTERS_DTYPES as DTYPES, CLUSTERS_NAMES as NAMES, check_clusters as check, float_bits as bits, restate_clusters as restate
from tests.sensing_common import SWEEP, chain_scene, make_sim, sweep_scene, wall_scene

pytestmark = pytest.mark.gpu

NAN = float('nan')


def three_in_four(E, N, rng_seed=16):
    return np.random.RandomState(rng_seed).rand(E, N) < 0.75


@pytest.mark.parametrize('E,N,R', SWEEP)
def test_clusters_equal_the_restatement(E, N, R):
    """N = 1, a partial tile, 333, four full tiles (a lane owns four kilobots), a radius beyond the arena; everybody and a
    random 3 in 4.  Every subset of the optional outputs gives the same label, and an output that is not asked for goes to
    the library as NULL."""
    g = make_sim(E, N, *sweep_scene(E, N))
    inr = ranges(g, R)
    for select in (None, three_in_four(E, N)):
        want = check(g, inr, R, select, what='sweep')
        if N == 1 and select is None:
            assert want[3].tolist() == [[1, 1, 0, 1]] * E
        s = None if select is None else dev(select)
        spy = Spy(g._lib)
        g._lib = spy
        try:
            results = [g.clusters(R, select=s, **dict(zip(NAMES[1:], on))) for on in itertools.product((False, True), repeat=3)]
        finally:
            g._lib = spy.lib
        calls = [a for n, a in spy.calls if n == 'kb_sense_clusters']
        assert len(calls) == 8 and all(a[3] is not None for a in calls) and all((a[2] is None) == (select is None) for a in calls)
        assert [tuple(a[4 + k] is not None for k in range(3)) for a in calls] == list(itertools.product((False, True), repeat=3))
        for on, res in zip(itertools.product((False, True), repeat=3), results):
            res = (res,) if torch.is_tensor(res) else res
            assert len(res) == 1 + sum(on)
            kept = [want[0]] + [w for w, o in zip(want[1:], on) if o]
            assert all(np.array_equal(bits(cpu(t)), bits(w)) for t, w in zip(res, kept)), on


def test_a_permuted_chain_of_1024():
    """The serpentine with its indices permuted: one component whose label is 0 in env 0 -- every kilobot ends under the one
    root, through the deepest hooking there is -- and sixteen runs of 63 with every 64th chain position unselected in env 1."""
    xy, pos = chain_scene()
    g = make_sim(2, 1024, xy, np.zeros((2, 1024)))
    R = 0.045
    inr = ranges(g, R)
    assert all(m.sum() == 2046 and m.sum(1).max() == 2 for m in inr)
    label, size, table, stats = check(g, inr, R, what='chain')
    assert (label == 0).all() and (size == 1024).all() and stats.tolist() == [[1, 1024, 0, 0]] * 2
    select = np.ones((2, 1024), dtype=bool)
    select[1] = pos % 64 != 63
    label, size, table, stats = check(g, inr, R, select, what='chain, runs')
    assert stats[0].tolist() == [1, 1024, 0, 0] and stats[1, [0, 1, 3]].tolist() == [16, 63, 0]
    assert np.array_equal(size[1], np.where(select[1], 63, 0)) and len(np.unique(label[1])) == 17
    # ... and in the order of the chain, where every kilobot first hooks under its predecessor
    order = np.argsort(pos)
    g = make_sim(2, 1024, xy[:, order], np.zeros((2, 1024)))
    inr = ranges(g, R)
    label, size, table, stats = check(g, inr, R, np.stack([np.ones(1024, dtype=bool), np.arange(1024) % 64 != 63]), what='chain in order')
    assert (label[0] == 0).all() and np.array_equal(label[1], np.where(np.arange(1024) % 64 != 63, np.arange(1024) // 64 * 64, -1))


def test_a_pile_in_one_cell():
    """40 kilobots on one point and 24 around it: a clique on one long chain of one cell, every pair of it in range."""
    N, R = 64, 0.05
    rng = np.random.RandomState(3)
    xy = np.zeros((2, N, 2))
    xy[:, :40] = [0.31, -0.2]
    xy[:, 40:] = np.array([0.31, -0.2]) + rng.uniform(-0.03, 0.03, size=(2, 24, 2))
    g = make_sim(2, N, xy, np.zeros((2, N)))
    inr = ranges(g, R)
    assert all(m[:40, :40].sum() == 40 * 39 for m in inr)
    label, size, table, stats = check(g, inr, R, what='pile')
    assert (label == 0).all() and stats.tolist() == [[1, N, 0, 0]] * 2
    select = np.ones((2, N), dtype=bool)
    select[0, :39] = False              # the pile's highest index alone stands for it
    select[1, ::2] = False
    label, size, table, stats = check(g, inr, R, select, what='pile, part')
    assert (label[0, 39:] == 39).all() and stats[0].tolist() == [1, 25, 39, 0] and stats[1].tolist() == [1, 32, 1, 0]


def test_the_predicate_at_its_boundary():
    """On the floats read back from the device: a pair with d2 == R2, which is joined, and a pair with d2 one ulp above R2,
    which is not."""
    R = 0.04
    Rw = np.float32(R) * np.float32(25)
    R2 = Rw * Rw
    above = np.nextafter(R2, np.float32(np.inf))
    base = np.float32(10.0)
    lift = None
    for k in range(1, 1 << 16):
        ey = (base + np.float32(k * 2.0 ** -20)) - base
        if Rw * Rw + ey * ey == above:
            lift = base + np.float32(k * 2.0 ** -20)
            break
    assert lift is not None
    N = 8
    x = np.array([0.0, Rw, 0.0, Rw, -20.0, -20.0, 15.0, 20.0], dtype=np.float32)
    y = np.array([0.0, 0.0, base, lift, -15.0, -15.0 + 0.5, 5.0, 5.0], dtype=np.float32)
    g = make_sim(1, N)
    g.x.copy_(torch.from_numpy(x)[None])
    g.y.copy_(torch.from_numpy(y)[None])
    gx, gy = state(g)[:2]
    d2 = lambda i, j: (gx[0, j] - gx[0, i]) * (gx[0, j] - gx[0, i]) + (gy[0, j] - gy[0, i]) * (gy[0, j] - gy[0, i])
    assert d2(0, 1).dtype == np.float32 and d2(0, 1) == R2 and d2(2, 3) == above and above > R2
    inr = ranges(g, R)
    assert inr[0][0, 1] and not inr[0][2, 3]
    label, size, table, stats = check(g, inr, R, what='boundary')
    assert label[0].tolist() == [0, 0, 2, 3, 4, 4, 6, 7] and stats[0].tolist() == [6, 2, 0, 4]


@pytest.mark.parametrize('R', [0.04, 0.15])
def test_clusters_at_walls_and_corners(R):
    xy, th = wall_scene()
    g = make_sim(4, xy.shape[1], xy, th)
    x, y = state(g)[:2]
    assert (np.abs(x) > 25.0).any() and (np.abs(y) > 18.75).any()      # some kilobots are outside: their cells clamp
    inr = ranges(g, R)
    for select in (None, three_in_four(4, xy.shape[1])):
        want = check(g, inr, R, select, what='walls')
        assert (want[3][:, 0] >= 2).all() and (want[3][:, 1] >= 3).all()


def test_select_extremes():
    E, N, R = 3, 96, 0.07
    g = make_sim(E, N, *scenes.gaussian_spawn(E, N, sigma=0.12, seed=8))
    inr = ranges(g, R)
    select = np.zeros((E, N), dtype=np.uint8)
    select[1] = 1
    select[2, 5] = 0xFF
    label, size, table, stats = check(g, inr, R, select, what='extremes')
    assert (label[0] == -1).all() and (size[0] == 0).all() and (bits(table[0]) == 0).all() and stats[0].tolist() == [0, 0, -1, 0]
    assert all(np.array_equal(bits(a[1]), bits(b[1])) for a, b in zip(restate(g, inr), (label, size, table, stats)))
    assert stats[1, 0] >= 2 and stats[1, 1] >= 3
    assert stats[2].tolist() == [1, 1, 5, 1] and label[2, 5] == 5 and (np.delete(label[2], 5) == -1).all() and table[2, 5, 0] == 1.0
    # a bool tensor works as it stands
    got = g.clusters(R, select=dev(select != 0), size=True, table=True, stats=True)
    assert all(np.array_equal(bits(cpu(t)), bits(w)) for t, w in zip(got, (label, size, table, stats)))


def test_every_element_is_written_and_out_is_reused():
    E, N, R = 3, 333, 0.05
    g = make_sim(E, N, *scenes.gaussian_spawn(E, N, sigma=0.2, seed=4))
    inr = ranges(g, R)
    first, other = three_in_four(E, N), three_in_four(E, N, rng_seed=17)
    other[1] = False
    want = restate(g, inr, first)
    assert (want[0] < 0).any() and (want[3][:, 0] >= 2).all() and (want[3][:, 3] >= 1).all()
    out = tuple(torch.full(w.shape, 77, dtype=d, device='cuda') for w, d in zip(want, DTYPES))
    for _ in range(2):
        got = g.clusters(R, select=dev(first), size=True, table=True, stats=True, out=out)
        assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, out))
        assert all(np.array_equal(bits(cpu(t)), bits(w)) for t, w in zip(out, want))
    # another select into the same buffers, with an env that selects nobody: nothing of the earlier answer is left
    g.clusters(R, select=dev(other), size=True, table=True, stats=True, out=out)
    assert all(np.array_equal(bits(cpu(t)), bits(w)) for t, w in zip(out, restate(g, inr, other)))
    lone = torch.full((E, N), 77, dtype=torch.int32, device='cuda')
    assert g.clusters(R, out=lone).data_ptr() == lone.data_ptr() and np.array_equal(cpu(lone), restate(g, inr)[0])


def test_alongside_hops_on_the_device():
    """One seed per component, seeds = (label == arange), into hops() at the same radius: every kilobot's root is its label,
    and all are reached."""
    E, N, R = 3, 333, 0.05
    g = make_sim(E, N, *scenes.gaussian_spawn(E, N, sigma=0.2, seed=4))
    label, stats = g.clusters(R, stats=True)
    seeds = label == torch.arange(N, device='cuda', dtype=torch.int32)[None]
    hops, root, hstats = g.hops(seeds, R, root=True, stats=True)
    assert torch.equal(root, label) and bool((hstats[:, 0] == N).all()) and bool((stats[:, 0] == seeds.sum(1)).all())
    assert bool((stats[:, 0] >= 2).all()) and bool((hops > 0).any())


def test_side_stream_and_untouched_state():
    E, N, R = 3, 333, 0.08
    g = make_sim(E, N, *scenes.gaussian_spawn(E, N, sigma=0.15, seed=5))
    fields = ('x', 'y', 'theta', 'status')
    before = {f: getattr(g, f).clone() for f in fields}
    s = dev(three_in_four(E, N))
    kept = s.clone()
    want = g.clusters(R, select=s, size=True, table=True, stats=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = g.clusters(R, select=s, size=True, table=True, stats=True)
    side.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, want)) and bool((want[1] > 1).any())
    torch.cuda.synchronize()
    for f in fields:
        assert torch.equal(before[f].view(torch.uint8), getattr(g, f).view(torch.uint8)), f
    assert torch.equal(s.view(torch.uint8), kept.view(torch.uint8))


def test_a_shard_reproduces_its_rows():
    E, N, R = 4, 64, 0.07
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.12, seed=6)
    whole, shard = make_sim(E, N, xy, th), make_sim(2, N, xy[2:4], th[2:4])
    select = dev(three_in_four(E, N))
    assert len({bytes(cpu(select[e]).tobytes()) for e in range(E)}) == E       # the selects differ per env
    w = whole.clusters(R, select=select, size=True, table=True, stats=True)
    s = shard.clusters(R, select=select[2:4].contiguous(), size=True, table=True, stats=True)
    assert all(torch.equal(a[2:4].view(torch.int32), b.view(torch.int32)) for a, b in zip(w, s)) and bool((s[1] > 1).any())


def test_python_checks():
    E, N, R = 2, 64, 0.07
    g = make_sim(E, N, *scenes.gaussian_spawn(E, N, sigma=0.12, seed=6))
    s = torch.ones(E, N, dtype=torch.bool, device='cuda')
    for bad in (s.float(), s.int(), s.cpu(), s[:, :5], s[:1], s.view(-1), torch.zeros(N, E, dtype=torch.bool, device='cuda').t(), cpu(s)):
        with pytest.raises(ValueError):
            g.clusters(R, select=bad)
    for radius in (0.0, -1.0, NAN):
        with pytest.raises(ValueError):
            g.clusters(radius)
    label = torch.empty(E, N, dtype=torch.int32, device='cuda')
    stats = torch.empty(E, 4, dtype=torch.int32, device='cuda')
    table = torch.empty(E, N, 4, dtype=torch.float32, device='cuda')
    for bad in (label.float(), label[:, :5], label.cpu(), (label, stats), torch.empty(N, E, dtype=torch.int32, device='cuda').t()):
        with pytest.raises(ValueError):
            g.clusters(R, out=bad)
    for bad in (label, (label,), (label, label), (stats, label), (label, stats.long()), (label, torch.empty(E, 2, dtype=torch.int32, device='cuda'))):
        with pytest.raises(ValueError):
            g.clusters(R, stats=True, out=bad)
    off = torch.empty(E * N * 4 + 1, dtype=torch.float32, device='cuda')[1:].view(E, N, 4)
    for bad in ((label, off), (label, table.int()), (label, table[..., :3])):
        with pytest.raises(ValueError):
            g.clusters(R, table=True, out=bad)
    got = g.clusters(R, select=s, table=True, out=(label, table))
    assert got[0].data_ptr() == label.data_ptr() and got[1].data_ptr() == table.data_ptr() and float(table[..., 0].sum()) == E * N


def test_batched_env_clusters():
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    E, N = 4, 64
    env = BatchedKilobotsEnv(E, N, seed=3, spawn_std=0.12, comm_radius=0.07)
    plain = BatchedKilobotsEnv(E, N, seed=3, spawn_std=0.12)
    assert torch.equal(env.reset(), plain.reset())
    select = dev(three_in_four(E, N))
    got = env.clusters(select, size=True, table=True, stats=True)
    want = env.sim.clusters(0.07, select=select, size=True, table=True, stats=True)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, want)) and bool((got[1] > 1).any())
    x, y = state(env.sim)[:2]
    assert np.array_equal(cpu(env.clusters()), ref.restate(x, y, 0.07)[0])
    with pytest.raises(ValueError):
        plain.clusters()
