"""kb_sense_reduce on the GPU against the brute-force numpy restatement of its definition (tests/reduce_ref.py).

Everything is compared for equality of the bit patterns: the fixed-point sum is exact on the quantised messages, min / max
return a value heard unchanged, and the counts are kb_sense's.  No tolerances."""
import numpy as np
import pytest
import torch

from tests import reduce_ref as ref
from tests import scenes
from tests.gpu_common import Spy, cpu, dev, ranges, state
from tests.sensing_checks import check_reduce as check, messages
from tests.sensing_common import SWEEP, make_sim, sweep_scene, wall_scene

pytestmark = pytest.mark.gpu

OPS = ('sum', 'min', 'max')
INF, NAN = float('inf'), float('nan')


@pytest.mark.parametrize('E,N,R', SWEEP)
def test_reductions_equal_the_restatement(E, N, R):
    """N = 1 (the identities), a partial tile, 333, four full tiles (at 8 channels the largest LDS image), a radius beyond
    the arena; the three ops on rows of 1, 3 (padded to 4) and 8 words, of 2 and 4 on two shapes, and a [E, N] tensor."""
    g = make_sim(E, N, *sweep_scene(E, N))
    inr = ranges(g, R)
    widths = (1, 3, 8) + ((2, 4) if (E, N, R) in ((8, 64, 0.07), (3, 333, 0.034)) else ())
    for C in widths:
        values = messages(E, N, C, 100 + C)
        for op in OPS:
            out, cnt = check(g, inr, R, op, values, what='sweep')
            if N == 1:
                assert not cnt.any() and (ref.bits(out) == ref.bits(np.float32({'sum': 0.0, 'min': INF, 'max': -INF}[op]))).all()
            else:
                assert cnt.any()
    check(g, inr, R, 'sum', messages(E, N, 3, 7), scale=1000.0, what='scale 1000')          # not a power of two
    flat = messages(E, N, 0, 8)
    out, _ = check(g, inr, R, 'min', flat, what='[E, N]')
    assert out.shape == (E, N)


@pytest.mark.parametrize('R', [0.04, 0.15])
def test_reductions_at_walls_and_corners(R):
    xy, th = wall_scene()
    g = make_sim(4, xy.shape[1], xy, th)
    x, y = state(g)[:2]
    assert (np.abs(x) > 25.0).any() and (np.abs(y) > 18.75).any()      # some kilobots are outside
    inr = ranges(g, R)
    for op in OPS:
        out, cnt = check(g, inr, R, op, messages(4, xy.shape[1], 4, 11), what='walls')
        assert cnt.max() > 0


def test_a_pile_in_one_cell_and_sums_beyond_2_24():
    """40 kilobots on one point and 24 around it: one long chain in one cell.  Integer messages of 2^19 .. 2^20 with scale 1:
    the sums pass 2^24, where the int -> float conversion at write-out rounds (to nearest even)."""
    N, R = 64, 0.05
    rng = np.random.RandomState(3)
    xy = np.zeros((2, N, 2))
    xy[:, :40] = [0.31, -0.2]
    xy[:, 40:] = np.array([0.31, -0.2]) + rng.uniform(-0.03, 0.03, size=(2, 24, 2))
    g = make_sim(2, N, xy, np.zeros((2, N)))
    inr = ranges(g, R)
    values = rng.randint(2 ** 19, 2 ** 20, size=(2, N, 2)).astype(np.float32)
    acc = np.stack([inr[e].astype(np.int64) @ values[e].astype(np.int64) for e in range(2)])
    assert acc.max() > 2 ** 24 and (acc.astype(np.float32).astype(np.int64) != acc).any()      # some sums are not floats
    assert all(m[:40, :40].sum() == 40 * 39 for m in inr)
    out, cnt = check(g, inr, R, 'sum', values, scale=1.0, what='pile')
    assert np.array_equal(out, acc.astype(np.float32)) and cnt.min() >= 39
    for op in ('min', 'max'):
        check(g, inr, R, op, values, what='pile')


SPECIALS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF,
                     0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF], dtype=np.uint32).view(np.float32)
SPECIALS = np.concatenate([SPECIALS, np.array([3e38, -3e38, 1.0, -1.0, 0.5, 1.5, 2.5, -2.5], dtype=np.float32)])


@pytest.mark.parametrize('op', OPS)
def test_special_values(op):
    """+-0, +-inf, NaNs of both signs, denormals and +-3e38 in one env: min / max return the exact bit pattern heard (-0
    against +0 included), the sum clamps, drops the NaNs and rounds halves to even."""
    N, R = 48, 0.06
    xy, th = scenes.gaussian_spawn(2, N, sigma=0.05, seed=12)
    g = make_sim(2, N, xy, th)
    inr = ranges(g, R)
    rng = np.random.RandomState(13)
    values = SPECIALS[rng.randint(0, len(SPECIALS), size=(2, N, 4))]
    # a kilobot that hears only zeros of both signs, one that hears only NaNs: the order of the bit patterns decides
    values[0, :, 0] = np.where(np.arange(N) % 2 == 0, np.float32(0.0), np.float32(-0.0))
    values[0, :, 1] = np.where(np.arange(N) % 2 == 0, SPECIALS[4], SPECIALS[5])
    out, cnt = check(g, inr, R, op, values, scale=1.0, what='specials')
    heard_both = (inr[0][:, 0::2].any(1)) & (inr[0][:, 1::2].any(1))
    assert heard_both.sum() > N // 2 and cnt.max() > 10
    if op == 'min':
        assert (ref.bits(out[0, heard_both, 0]) == 0x80000000).all() and (ref.bits(out[0, heard_both, 1]) == 0xFFC00000).all()
    elif op == 'max':
        assert (ref.bits(out[0, heard_both, 0]) == 0).all() and (ref.bits(out[0, heard_both, 1]) == 0x7FC00000).all()
    else:
        assert (ref.bits(out[0, :, :2]) == 0).all()              # zeros and NaNs sum to +0.0
        assert np.isfinite(out).all()


def test_saturation_cannot_overflow():
    """The only shape at which the int32 sum could overflow: 1024 kilobots that all hear each other, every message clamped."""
    g = make_sim(1, 1024, *scenes.lattice_spawn(1, 1024, seed=3))
    values = torch.full((1, 1024, 3), 3e38, device='cuda')
    values[..., 1] = -INF
    values[..., 2] = NAN
    out, cnt = g.neighbor_reduce(values, 4.0, op='sum', scale=1.0, count=True)
    torch.cuda.synchronize()
    assert (cpu(cnt) == 1023).all()
    out = cpu(out)
    assert 1023 * 2 ** 21 == 2145386496 and float(np.float32(2145386496)) == 2145386496.0
    assert (out[..., 0] == np.float32(2145386496)).all() and (out[..., 1] == np.float32(-2145386496)).all()
    assert (ref.bits(out[..., 2]) == 0).all()
    want, _ = ref.restate(*state(g)[:2], cpu(values), 4.0, 'sum', 1.0)
    assert np.array_equal(ref.bits(out), ref.bits(want))


def test_outputs_in_place_streams_and_untouched_state():
    E, N, R, C = 3, 333, 0.08, 4
    g = make_sim(E, N, *scenes.gaussian_spawn(E, N, sigma=0.15, seed=5))
    fields = ('x', 'y', 'theta', 'status')
    before = {f: getattr(g, f).clone() for f in fields}
    inr = ranges(g, R)
    values = messages(E, N, C, 21)
    want = {op: np.stack([ref.reduce_env(inr[e], values[e], op)[0] for e in range(E)]) for op in OPS}
    wcnt = np.stack([m.sum(1) for m in inr]).astype(np.uint32)
    same = lambda t, w: np.array_equal(ref.bits(cpu(t)), ref.bits(w))
    v = dev(values)
    for op in OPS:
        # a buffer full of NaN comes back fully written; reused: the same answer twice
        out = torch.full((E, N, C), NAN, device='cuda')
        for _ in range(2):
            got = g.neighbor_reduce(v, R, op=op, out=out)
            assert got.data_ptr() == out.data_ptr() and same(out, want[op])
        # in place: the messages are replaced by what was heard
        buf = v.clone()
        got = g.neighbor_reduce(buf, R, op=op, out=buf)
        assert got.data_ptr() == buf.data_ptr() and same(buf, want[op])
    assert torch.equal(v.view(torch.int32), dev(values).view(torch.int32))
    # (result, count) into preallocated tensors; 8 channels in place, with the count
    out = torch.full((E, N, C), NAN, device='cuda')
    cnt = torch.full((E, N), 77, dtype=torch.int32, device='cuda')
    o2, c2 = g.neighbor_reduce(v, R, out=(out, cnt), count=True)
    assert o2.data_ptr() == out.data_ptr() and c2.data_ptr() == cnt.data_ptr()
    assert same(o2, want['sum']) and np.array_equal(cpu(c2).view(np.uint32), wcnt)
    wide = messages(E, N, 8, 22)
    buf = dev(wide)
    g.neighbor_reduce(buf, R, op='max', out=(buf, cnt), count=True)
    assert same(buf, np.stack([ref.reduce_env(inr[e], wide[e], 'max')[0] for e in range(E)]))
    # count=False hands the library NULL for d_count
    spy = Spy(g._lib)
    g._lib = spy
    try:
        only = g.neighbor_reduce(v, R)
        g.neighbor_reduce(v, R, count=True)
    finally:
        g._lib = spy.lib
    calls = [a for n, a in spy.calls if n == 'kb_sense_reduce']
    assert len(calls) == 2 and calls[0][7] is None and calls[1][7] is not None
    assert torch.is_tensor(only) and same(only, want['sum'])
    # a side stream gives the default stream's answer
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        os_, cs = g.neighbor_reduce(v, R, op='min', count=True)
    side.synchronize()
    assert same(os_, want['min']) and np.array_equal(cpu(cs).view(np.uint32), wcnt)
    # the call reads the state and writes its outputs only
    torch.cuda.synchronize()
    for f in fields:
        assert torch.equal(before[f].view(torch.uint8), getattr(g, f).view(torch.uint8)), f
    # arguments are checked before the call
    for bad in (v.double(), v.cpu(), v[..., :3], v.transpose(0, 1), v[:, :5], torch.zeros(E, N, 9, device='cuda'), torch.zeros(E, device='cuda'), values):
        with pytest.raises(ValueError):
            g.neighbor_reduce(bad, R)
    for bad in (out.view(E, N * C), out.double(), out[..., :3], (out, cnt)):
        with pytest.raises(ValueError):
            g.neighbor_reduce(v, R, out=bad)
    for bad in (out, (out,), (out, cnt.float())):
        with pytest.raises(ValueError):
            g.neighbor_reduce(v, R, out=bad, count=True)
    for kw in (dict(op='mean'), dict(op=3), dict(scale=0.0), dict(scale=NAN), dict(scale=INF)):
        with pytest.raises(ValueError):
            g.neighbor_reduce(v, R, **kw)
    for radius in (0.0, -1.0, NAN):
        with pytest.raises(ValueError):
            g.neighbor_reduce(v, radius)


def test_a_shard_reproduces_its_rows():
    E, N, R = 4, 64, 0.07
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.12, seed=6)
    whole, shard = make_sim(E, N, xy, th), make_sim(2, N, xy[2:4], th[2:4])
    values = dev(messages(E, N, 3, 31))
    for op in OPS:
        ow, cw = whole.neighbor_reduce(values, R, op=op, scale=1000.0, count=True)
        os_, cs = shard.neighbor_reduce(values[2:4].contiguous(), R, op=op, scale=1000.0, count=True)
        assert torch.equal(ow[2:4].contiguous().view(torch.int32), os_.view(torch.int32)) and torch.equal(cw[2:4], cs)
        assert bool(cs.any())


def test_hop_count_on_the_device():
    """h <- min(h, reduce_min(h) + 1), the reduction in place on a scratch copy, the + 1 in torch: after 20 sweeps (the deepest
    hop of the scene is 15) the hop counts are those of a breadth-first search, kilobots out of reach stay +inf."""
    N, R = 333, 0.05
    g = make_sim(1, N, *scenes.gaussian_spawn(1, N, sigma=0.2, seed=4))
    x, y = state(g)[:2]
    want = ref.breadth_first(ref.in_range(x[0], y[0], R))
    reached = np.isfinite(want)
    assert reached.sum() > 100 and (~reached).any() and want[reached].max() < 20
    h = torch.full((1, N), INF, device='cuda')
    h[0, 0] = 0.0
    buf = torch.empty_like(h)
    for _ in range(20):
        buf.copy_(h)
        g.neighbor_reduce(buf, R, op='min', out=buf)
        h = torch.minimum(h, buf + 1.0)
    assert np.array_equal(cpu(h)[0], want)


def test_batched_env_neighbor_reduce():
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    E, N = 4, 64
    env = BatchedKilobotsEnv(E, N, seed=3, spawn_std=0.12, comm_radius=0.07)
    plain = BatchedKilobotsEnv(E, N, seed=3, spawn_std=0.12)
    assert torch.equal(env.reset(), plain.reset())
    a = dev(scenes.random_actions(E, N, seed=20))
    obs, _, _, info = env.step(a)
    assert info == {} and torch.equal(obs, plain.step(a)[0])
    values = dev(messages(E, N, 4, 41))
    for op in OPS:
        got, cnt = env.neighbor_reduce(values, op=op, count=True)
        want, wcnt = env.sim.neighbor_reduce(values, 0.07, op=op, count=True)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(cnt, wcnt) and bool(cnt.any())
    inr = ranges(env.sim, 0.07)
    assert np.array_equal(ref.bits(cpu(env.neighbor_reduce(values, scale=1000.0))),
                          ref.bits(np.stack([ref.reduce_env(inr[e], cpu(values)[e], 'sum', 1000.0)[0] for e in range(E)])))
    with pytest.raises(ValueError):
        plain.neighbor_reduce(values)
