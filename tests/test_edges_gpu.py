"""kb_sense_edges on the GPU against the numpy restatement of its definition (tests/edges_ref.py): brute force over all pairs
of an env, np.nonzero for the ascending rows.

Everything is compared for equality: node ids, counts and offsets as integers, rel by its bit patterns.  No tolerances.  The
memory contract is tested as defined behaviour: the outputs lie between sentinel words, the offsets are stale or the capacity
is off, every store stays inside the buffers, and the outputs equal edges_ref.contract.  That the scenes are not vacuous --
rows above 16, empty rows, a batch without an edge, complete rows -- is asserted on the restatement alone in
tests/test_edges_cpu.py."""
import numpy as np
import pytest
import torch

from tests import edges_ref as ref
from tests import geometry_scenes as GS
from tests import scenes
from tests.gpu_common import cpu, dev, geometry_pair, state
from tests.sensing_common import SWEEP, make_sim, sweep_scene, wall_scene

pytestmark = pytest.mark.gpu

SENTINEL = -77
PAD = 64            # sentinel slots in front of and behind every output of the memory-contract tests
STATE = ('x', 'y', 'theta', 'v', 'w', 'status', 'ws_cnt', 'ws_key', 'ws_acc', 'scratch')


def ubits(t):
    return cpu(t).view(np.uint32)


def check(g, R, what=''):
    """edges(R) against the restatement on the state of the sim as it is on the device.  Returns the restatement."""
    E, N = g.num_envs, g.num_bots
    got = g.edges(R)
    sensed = g.sense(R)
    torch.cuda.synchronize()
    true = ref.restate(*state(g), R)
    wsrc, wdst, wrel, wcount, woff = true
    nnz = len(wsrc)
    print('%s E=%d N=%d R=%g: nnz %d (device %s), longest row %d' % (what, E, N, R, nnz, got.nnz, int(wcount.max())))
    assert type(got).__name__ == 'Edges' and got._fields == ('src', 'dst', 'rel', 'offsets', 'count', 'nnz')
    assert isinstance(got.nnz, int) and got.nnz == nnz, what
    assert got.src.dtype == got.dst.dtype == got.count.dtype == torch.int32 and got.rel.dtype == torch.float32 and got.offsets.dtype == torch.int64
    assert tuple(got.src.shape) == tuple(got.dst.shape) == (nnz,) and tuple(got.rel.shape) == (nnz, 4)
    assert tuple(got.offsets.shape) == (E * N + 1,) and tuple(got.count.shape) == (E, N)
    assert np.array_equal(ubits(got.count), wcount), what
    assert np.array_equal(ubits(got.count), ubits(sensed)), what
    assert np.array_equal(cpu(got.offsets), woff), what
    bad = np.flatnonzero(cpu(got.dst) != wdst)
    assert len(bad) == 0, (what, bad[:5], cpu(got.dst)[bad[:5]], wdst[bad[:5]])
    assert np.array_equal(cpu(got.src), wsrc), what
    assert np.array_equal(ubits(got.rel), ref.bits(wrel)), what
    return true


@pytest.mark.parametrize('E,N,R', SWEEP)
def test_edges_equal_the_restatement(E, N, R):
    """The sweep of the sensing kernels: cfg2 / cfg3 slices, odd sizes, one kilobot (nnz == 0), radii from below a cell to
    beyond the arena; (2, 7, 4.0) is the shape on which the entry points clamp the reach to the whole grid."""
    xy, th = sweep_scene(E, N)
    g = make_sim(E, N, xy, th)
    count = check(g, R, 'sweep')[3]
    assert count.max() > 0 or N == 1


@pytest.mark.parametrize('R', [0.04, 0.09, 0.15])
def test_edges_at_walls_and_corners(R):
    xy, th = wall_scene(random_headings=True)
    g = make_sim(4, xy.shape[1], xy, th)
    x, y = state(g)[:2]
    assert (np.abs(x) > 25.0).any() and (np.abs(y) > 18.75).any()      # some kilobots are outside: their cell indices clamp
    check(g, R, 'walls')


@pytest.mark.parametrize('N', [32, 33, 65, 257, 1024])
def test_complete_graphs(N):
    """Every kilobot sees every other: rows of N - 1 across the mask-word boundary (32 | 33), the 64-lane boundary, the 256-row
    tile boundary, and the full 1023-neighbour rows of 1024 kilobots."""
    xy, th = sweep_scene(2, N)
    g = make_sim(2, N, xy, th)
    count = check(g, 4.0, 'complete')[3]
    assert (count == N - 1).all()


def pile_sim():
    E, N = 2, 200
    rng = np.random.RandomState(17)
    xy = rng.uniform(-0.6, 0.6, size=(E, N, 2))
    xy[0, :150] = (0.3123, -0.2011)                 # env 0: kilobots 0 .. 149 on one point
    xy[1, 25:175] = (-0.9871, 0.7433)               # env 1: kilobots 25 .. 174, in the corner cell
    return make_sim(E, N, xy, rng.uniform(-np.pi, np.pi, size=(E, N)))


def test_a_pile_is_ordered_by_index_alone():
    """150 kilobots at exactly the same point: one long chain in one cell, rows of at least 149 entries with d2 == 0, which
    nothing but ascending j orders."""
    g = pile_sim()
    src, dst, rel, count, off = check(g, 0.07, 'pile')
    for e, first in ((0, 0), (1, 25)):
        rows = np.arange(first, first + 150) + e * 200
        assert (count.ravel()[rows] >= 149).all()
        for r in rows[[0, 1, 77, 149]]:
            row = slice(int(off[r]), int(off[r + 1]))
            zero = rel[row, 2] == 0
            assert zero.sum() == 149 and np.array_equal(dst[row][zero], rows[rows != r])
            assert (np.diff(dst[row]) > 0).all()


@pytest.mark.parametrize('E,N,R', [(8, 64, 0.07), (8, 64, 0.3), (3, 333, 0.034), (4, 1024, 0.1)])
def test_short_rows_equal_the_neighbour_lists(E, N, R):
    """On the device alone: for every row of at most 16 entries, the set of (j, rel bits) of neighbors(R, 16) is the row."""
    xy, th = sweep_scene(E, N)
    g = make_sim(E, N, xy, th)
    ed = g.edges(R)
    index, nrel, ncount = g.neighbors(R, 16)
    torch.cuda.synchronize()
    assert torch.equal(ed.count, ncount)
    count, off = cpu(ed.count).ravel(), cpu(ed.offsets)
    dst, rel = cpu(ed.dst), ubits(ed.rel)
    index, nrel = cpu(index).reshape(E * N, 16), ubits(nrel).reshape(E * N, 16, 4)
    short = np.flatnonzero(count <= 16)
    assert len(short) > 0 and (count[short] > 0).any()
    for r in short:
        m, lo = int(count[r]), int(off[r])
        order = np.argsort(index[r, :m])                # the list is ordered by (d2, j), the row by j
        assert np.array_equal(index[r, :m][order] + (r // N) * N, dst[lo:lo + m]), r
        assert np.array_equal(nrel[r, :m][order], rel[lo:lo + m]), r


# ---- the memory contract ---------------------------------------------------------------------------------------------------
def guarded(capacity):
    """src, dst, rel of `capacity` slots between PAD sentinel slots on either side: (whole tensors, the views to hand over)."""
    whole = (torch.full((capacity + 2 * PAD,), SENTINEL, dtype=torch.int32, device='cuda'),
             torch.full((capacity + 2 * PAD,), SENTINEL, dtype=torch.int32, device='cuda'),
             torch.full((capacity + 2 * PAD, 4), float(SENTINEL), device='cuda'))
    views = tuple(t[PAD:PAD + capacity] for t in whole)
    assert views[2].data_ptr() % 16 == 0
    return whole, views


def run_contract(g, R, true, offsets, capacity, what):
    """One raw call with the given offsets and capacity into guarded buffers, against edges_ref.contract."""
    E, N = g.num_envs, g.num_bots
    whole, (src, dst, rel) = guarded(capacity)
    count = torch.full((E, N), SENTINEL, dtype=torch.int32, device='cuda')
    g._sense_edges(R, dev(offsets), capacity, src, dst, rel, count)
    torch.cuda.synchronize()
    before = (np.full(capacity, SENTINEL, np.int32), np.full(capacity, SENTINEL, np.int32), np.full((capacity, 4), SENTINEL, np.float32))
    wsrc, wdst, wrel, owned = ref.contract(true, offsets, capacity, before)
    print('%s: capacity %d, nnz %d, %d slots owned, %d filled with -1' % (what, capacity, len(true[0]), owned.sum(), (wdst == -1).sum()))
    for t in whole:
        t = cpu(t)
        assert (t[:PAD] == SENTINEL).all() and (t[PAD + capacity:] == SENTINEL).all(), what       # in front of the buffer and behind it
    assert np.array_equal(cpu(dst), wdst) and np.array_equal(cpu(src), wsrc), what
    assert np.array_equal(ubits(rel), ref.bits(wrel)), what
    assert (cpu(dst)[~owned] == SENTINEL).all() and (cpu(src)[~owned] == SENTINEL).all() and (cpu(rel)[~owned] == SENTINEL).all(), what
    assert np.array_equal(ubits(count), true[3]), what                  # the true counts, whatever the offsets say
    return wdst, owned


@pytest.fixture(scope='module')
def contract_scene():
    """(8, 64) at 0.3 m -- rows of up to 48 -- with the restatement, and the offsets of OTHER poses (the next seed)."""
    E, N, R = 8, 64, 0.3
    xy, th = sweep_scene(E, N)
    g = make_sim(E, N, xy, th)
    true = ref.restate(*state(g), R)
    other = ref.restate(*ref.world(*scenes.gaussian_spawn(E, N, sigma=0.2, seed=5)), R)
    return g, R, true, other


def test_stale_offsets_stay_inside_their_rows(contract_scene):
    """Offsets of other poses: some rows are too short (their tail is dropped), some too long (-1 / 0 behind the row); the
    stale total is below or above the capacity."""
    g, R, true, other = contract_scene
    stale, nnz = other[4], len(true[0])
    slots, count = np.diff(stale), true[3].ravel().astype(np.int64)
    assert (slots < count).any() and (slots > count).any()
    for capacity in (nnz, int(stale[-1]), int(stale[-1]) - 1000):
        wdst, owned = run_contract(g, R, true, stale, capacity, 'stale offsets')
        assert (wdst[owned] == -1).any() and (wdst[owned] >= 0).any()
    # shifted down: negative in front, one row 700 slots too long, beyond the capacity behind
    shifted = true[4] - 500
    shifted[300:] += 700
    wdst, owned = run_contract(g, R, true, shifted, nnz, 'shifted down')
    assert owned.all() and (wdst == -1).sum() == 700
    # shifted up: the slots in front of the first row and behind the last belong to no row
    wdst, owned = run_contract(g, R, true, true[4] + 500, nnz + 800, 'shifted up')
    assert not owned[:500].any() and owned[500:nnz + 500].all() and not owned[nnz + 500:].any()
    assert np.array_equal(wdst[500:nnz + 500], true[1])


def test_a_capacity_below_and_above_nnz(contract_scene):
    g, R, true, _ = contract_scene
    nnz = len(true[0])
    for capacity in (nnz - 1, nnz // 2 + 7, 1):
        wdst, owned = run_contract(g, R, true, true[4], capacity, 'below')
        assert owned.all() and np.array_equal(wdst, true[1][:capacity])
    for capacity in (nnz, nnz + 1, nnz + 333):
        wdst, owned = run_contract(g, R, true, true[4], capacity, 'above')
        assert owned.sum() == nnz and np.array_equal(wdst[:nnz], true[1]) and (wdst[nnz:] == SENTINEL).all()


def test_python_capacity_path_reads_nothing_back(contract_scene):
    g, R, true, _ = contract_scene
    nnz = len(true[0])
    for capacity in (nnz + 100, nnz - 100):
        ed = g.edges(R, capacity=capacity)
        assert torch.is_tensor(ed.nnz) and ed.nnz.is_cuda and ed.nnz.dim() == 0 and ed.nnz.dtype == torch.int64 and int(ed.nnz) == nnz
        assert tuple(ed.dst.shape) == tuple(ed.src.shape) == (capacity,) and tuple(ed.rel.shape) == (capacity, 4)
        m = min(capacity, nnz)
        assert np.array_equal(cpu(ed.dst)[:m], true[1][:m]) and np.array_equal(cpu(ed.src)[:m], true[0][:m])
        assert np.array_equal(ubits(ed.rel)[:m], ref.bits(true[2])[:m])
        assert (cpu(ed.dst)[m:] == -1).all() and (cpu(ed.src)[m:] == -1).all() and (ubits(ed.rel)[m:] == 0).all()
        assert np.array_equal(cpu(ed.offsets), true[4]) and np.array_equal(ubits(ed.count), true[3])


def test_optional_outputs_leave_the_others_alone(contract_scene):
    g, R, true, _ = contract_scene
    full = g.edges(R)
    no_src, no_rel, neither = g.edges(R, src=False), g.edges(R, rel=False), g.edges(R, src=False, rel=False)
    assert no_src.src is None and no_rel.rel is None and neither.src is None and neither.rel is None
    for ed in (no_src, no_rel, neither):
        assert torch.equal(ed.dst, full.dst) and torch.equal(ed.offsets, full.offsets) and torch.equal(ed.count, full.count) and ed.nnz == full.nnz
    assert torch.equal(no_src.rel.view(torch.int32), full.rel.view(torch.int32)) and torch.equal(no_rel.src, full.src)
    # count only: through Python (empty lists, the counts from sense) and as the counting call of the library itself
    only = g.edges(R, capacity=0)
    assert only.dst.numel() == only.src.numel() == only.rel.numel() == 0 and int(only.nnz) == full.nnz
    assert torch.equal(only.count, full.count) and torch.equal(only.offsets, full.offsets)
    count = torch.full((g.num_envs, g.num_bots), SENTINEL, dtype=torch.int32, device='cuda')
    g._sense_edges(R, full.offsets, 0, None, None, None, count)
    assert torch.equal(count, full.count)
    g._sense_edges(R, full.offsets, 0, None, None, None, None)         # nothing to write: KB_OK, nothing launched


def test_the_call_reads_the_state_and_writes_its_outputs_only():
    E, N = 4, 96
    xy, th = wall_scene(random_headings=True)
    g = make_sim(E, N, xy, th)
    a = torch.zeros(E, N, 2, device='cuda')
    a[..., 0] = 0.01
    g.step(5, actions=a)                    # (leaves a contact store behind)
    torch.cuda.synchronize()
    before = {f: getattr(g, f).clone() for f in STATE}
    ed = g.edges(0.15)
    offsets = ed.offsets.clone()
    g._sense_edges(0.15, ed.offsets, ed.nnz, ed.src, ed.dst, ed.rel, ed.count)
    torch.cuda.synchronize()
    assert ed.nnz > 0 and torch.equal(offsets, ed.offsets)
    for f in STATE:
        assert torch.equal(before[f].view(torch.uint8), getattr(g, f).view(torch.uint8)), f
    check(g, 0.15, 'after a step')


def test_calling_twice_gives_the_same_bits_on_any_stream():
    xy, th = sweep_scene(8, 64)
    g = make_sim(8, 64, xy, th)
    first, second = g.edges(0.3), g.edges(0.3)
    assert first.dst.data_ptr() != second.dst.data_ptr()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        third = g.edges(0.3)
    side.synchronize()
    for ed in (second, third):
        assert ed.nnz == first.nnz and torch.equal(ed.src, first.src) and torch.equal(ed.dst, first.dst)
        assert torch.equal(ed.rel.view(torch.int32), first.rel.view(torch.int32)) and torch.equal(ed.offsets, first.offsets)


def test_preallocated_outputs_are_reused_and_checked():
    xy, th = sweep_scene(8, 64)
    g = make_sim(8, 64, xy, th)
    full = g.edges(0.3)
    n = full.nnz
    src, dst = (torch.full((n,), SENTINEL, dtype=torch.int32, device='cuda') for _ in range(2))
    rel = torch.full((n, 4), float(SENTINEL), device='cuda')
    got = g.edges(0.3, out=(src, dst, rel))
    assert got.src.data_ptr() == src.data_ptr() and got.dst.data_ptr() == dst.data_ptr() and got.rel.data_ptr() == rel.data_ptr()
    assert torch.equal(src, full.src) and torch.equal(dst, full.dst) and torch.equal(rel.view(torch.int32), full.rel.view(torch.int32))
    dst.fill_(SENTINEL)
    assert g.edges(0.3, src=False, rel=False, out=dst).dst.data_ptr() == dst.data_ptr() and torch.equal(dst, full.dst)
    big = torch.full((n + 5,), SENTINEL, dtype=torch.int32, device='cuda')
    got = g.edges(0.3, capacity=n + 5, src=False, rel=False, out=(big,))
    assert torch.equal(big[:n], full.dst) and bool((big[n:] == SENTINEL).all())         # behind nnz the caller's tensor is left alone
    for bad in (dst, (src, dst), (src, dst, rel, rel), (src, dst.long(), rel), (src.cpu(), dst, rel), (src, dst[:-1], rel), (src, dst, rel[:, :3]),
                (src, dst, rel.view(4, n).t())):
        with pytest.raises(ValueError):
            g.edges(0.3, out=bad)
    for args in ((0.0,), (-1.0,), (0.3, -1), (0.3, 1.5)):
        with pytest.raises(ValueError):
            g.edges(*args)
    # on a bound handle a d_rel off its 16 bytes is an argument error, and nothing is written
    from gym_kilobots_amd import _native as nat
    odd = torch.zeros(4 * n + 4, device='cuda')[1:4 * n + 1]
    dst.fill_(SENTINEL)
    with pytest.raises(nat.KilobotsHipError, match='16-byte aligned'):
        g._sense_edges(0.3, full.offsets, n, None, dst, odd, None)
    assert odd.data_ptr() % 16 == 4 and bool((dst == SENTINEL).all())
    # the raw call refuses tensors the capacity or the rows do not fit into, before the library sees them
    for bad in ((full.offsets, n + 1, None, dst, None, None), (full.offsets[:-1], n, None, dst, None, None), (full.offsets.int(), n, None, dst, None, None),
                (full.offsets, n, src[:-1], dst, None, None), (full.offsets, n, None, dst, rel[:-1], None), (full.offsets, n, None, dst, None, full.count[:-1])):
        with pytest.raises(ValueError):
            g._sense_edges(0.3, *bad)
    assert bool((dst == SENTINEL).all())


def test_a_shard_reproduces_its_rows():
    """Two sims of two envs against the sim of four: the same rows, up to the base of the row pointer and of the node ids."""
    E, N = 4, 96
    xy, th = wall_scene(random_headings=True)
    whole = make_sim(E, N, xy, th).edges(0.15)
    woff = cpu(whole.offsets)
    for k in (0, 1):
        shard = make_sim(2, N, xy[2 * k:2 * k + 2], th[2 * k:2 * k + 2]).edges(0.15)
        lo, hi = int(woff[2 * k * N]), int(woff[(2 * k + 2) * N])
        assert shard.nnz == hi - lo > 0
        assert np.array_equal(cpu(shard.offsets), woff[2 * k * N:(2 * k + 2) * N + 1] - lo)
        assert torch.equal(shard.src + 2 * k * N, whole.src[lo:hi]) and torch.equal(shard.dst + 2 * k * N, whole.dst[lo:hi])
        assert torch.equal(shard.rel.view(torch.int32), whole.rel[lo:hi].contiguous().view(torch.int32))
        assert torch.equal(shard.count, whole.count[2 * k:2 * k + 2])


@pytest.mark.parametrize('row', GS.SENSING_ROWS, ids=lambda g: g.name)
def test_edges_off_the_default_arena(row):
    """The arenas of tests/geometry_scenes.py that the sensing kernels are run on: cells of 0.875, 1.75 and 3.5, 103 x 78 cells
    with 1024 kilobots (the largest LDS image), grids one and two cells thin.  A radius of a cell and a half of the row's own cell."""
    _, _, g = geometry_pair(row)
    check(g, GS.sensing_radius(row, 'cell-and-a-half'), row.name)


def test_batched_env_edge_obs():
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    E, N = 4, 64
    spawn = dict(seed=3, spawn_std=0.12)
    env = BatchedKilobotsEnv(E, N, edge_obs=0.1, **spawn)
    fixed = BatchedKilobotsEnv(E, N, edge_obs=(0.1, 20000), **spawn)
    plain = BatchedKilobotsEnv(E, N, **spawn)
    assert env.edge_obs == (0.1, None) and fixed.edge_obs == (0.1, 20000) and plain.edge_obs is None
    first = plain.reset()
    assert torch.equal(env.reset(), first) and torch.equal(fixed.reset(), first)
    a = dev(scenes.random_actions(E, N, seed=20))
    obs, _, _, info = env.step(a)
    fobs, _, _, finfo = fixed.step(a)
    pobs, _, _, pinfo = plain.step(a)
    assert pinfo == {} and torch.equal(obs, pobs) and torch.equal(fobs, pobs)
    assert sorted(info) == ['edges'] and sorted(finfo) == ['edges']
    true = check(env.sim, 0.1, 'env')
    nnz = len(true[0])
    assert 0 < nnz < 20000
    for got in (info['edges'], env.edges()):
        assert got.nnz == nnz and np.array_equal(cpu(got.dst), true[1]) and np.array_equal(cpu(got.src), true[0])
        assert np.array_equal(ubits(got.rel), ref.bits(true[2]))
    got = finfo['edges']
    assert torch.is_tensor(got.nnz) and int(got.nnz) == nnz and tuple(got.dst.shape) == (20000,)
    assert np.array_equal(cpu(got.dst)[:nnz], true[1]) and (cpu(got.dst)[nnz:] == -1).all()
    with pytest.raises(ValueError):
        plain.edges()
    for bad in (0.0, (0.1, -1), (0.1, 8, 1)):
        with pytest.raises(ValueError):
            BatchedKilobotsEnv(E, N, edge_obs=bad)
