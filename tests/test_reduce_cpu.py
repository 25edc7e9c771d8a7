"""kb_sense_reduce without a GPU: the symbol is exported and bound, the host-side validation answers in the header's order
(arguments before the bound check, so none of it needs a device), no instantiation of the kernel has a private segment or a
spill (the code object's metadata), the numpy restatement (tests/reduce_ref.py) is the intended quantity -- a sum within
its quantisation bound, order-independent reductions, a hop count that equals a breadth-first search -- and
BatchedKilobotsEnv checks comm_radius at construction."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from tests import reduce_ref as ref
from tests import scenes
from tests.host_common import handle, lib  # noqa: F401
from tests.sensing_common import kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float('inf'), float('nan')


def test_symbol_is_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, 'include', 'kilobots_hip.h')).read()
    assert re.search(r'\bint\s+kb_sense_reduce\s*\(', hdr)
    assert 'kb_sense_reduce' in nat.EXPORTS and hasattr(lib, 'kb_sense_reduce')
    assert lib.kb_sense_reduce.argtypes is not None and len(lib.kb_sense_reduce.argtypes) == 9
    assert set(re.findall(r'\b(kb_[a-z_]+)\s*\(', hdr)) == set(nat.EXPORTS)
    m = re.search(r'#define\s+KB_REDUCE_MAX_CHANNELS\s+(\d+)', hdr)
    assert m and int(m.group(1)) == nat.REDUCE_MAX_CHANNELS == 8
    for name, value in (('KB_REDUCE_SUM', nat.REDUCE_SUM), ('KB_REDUCE_MIN', nat.REDUCE_MIN), ('KB_REDUCE_MAX', nat.REDUCE_MAX)):
        m = re.search(r'\b' + name + r'\s*=\s*(\d+)', hdr)
        assert m and int(m.group(1)) == value, name
    assert (nat.REDUCE_SUM, nat.REDUCE_MIN, nat.REDUCE_MAX) == (ref.SUM, ref.MIN, ref.MAX) == (0, 1, 2)


def test_validation_on_an_unbound_handle(lib, handle):
    """Nothing here launches: the pointers are never dereferenced on the host (any non-NULL value will do)."""
    val, out, cnt = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)
    S, MN = nat.REDUCE_SUM, nat.REDUCE_MIN
    bad = [
        ('op = -1', (handle, 0.07, -1, 4, 65536.0, val, out, cnt, None)),
        ('op = 3', (handle, 0.07, 3, 4, 65536.0, val, out, cnt, None)),
        ('channels = 0', (handle, 0.07, S, 0, 65536.0, val, out, cnt, None)),
        ('channels = 9', (handle, 0.07, MN, 9, 65536.0, val, out, cnt, None)),
        ('radius = 0', (handle, 0.0, S, 4, 65536.0, val, out, cnt, None)),
        ('radius = -1', (handle, -1.0, MN, 4, 65536.0, val, out, cnt, None)),
        ('radius = NaN', (handle, NAN, S, 4, 65536.0, val, out, cnt, None)),
        ('sum, scale = 0', (handle, 0.07, S, 4, 0.0, val, out, cnt, None)),
        ('sum, scale = -1', (handle, 0.07, S, 4, -1.0, val, out, cnt, None)),
        ('sum, scale = inf', (handle, 0.07, S, 4, INF, val, out, cnt, None)),
        ('sum, scale = NaN', (handle, 0.07, S, 4, NAN, val, out, cnt, None)),
        ('NULL sim', (None, 0.07, S, 4, 65536.0, val, out, cnt, None)),
        ('NULL d_values', (handle, 0.07, S, 4, 65536.0, None, out, cnt, None)),
        ('NULL d_out', (handle, 0.07, S, 4, 65536.0, val, None, cnt, None)),
    ]
    for what, args in bad:
        lib.kb_sense_neighbors(None, 0.07, 8, val, val, cnt, None)     # (leaves a message that the next call must replace)
        assert lib.kb_sense_reduce(*args) == nat.KB_EINVAL, what
        msg = lib.kb_last_error()
        assert msg and b'kb_sense_reduce' in msg, what
    # legal arguments reach the bound check: every op and channel count, d_count optional, min / max whatever the scale
    for op in (nat.REDUCE_SUM, nat.REDUCE_MIN, nat.REDUCE_MAX):
        for channels in range(1, 9):
            for c in (cnt, None):
                assert lib.kb_sense_reduce(handle, 0.07, op, channels, 1000.0, val, out, c, None) == nat.KB_ENOTBOUND
                assert b'kb_sense_reduce' in lib.kb_last_error() and b'kb_bind' in lib.kb_last_error()
    for scale in (NAN, 0.0, -1.0, INF):
        assert lib.kb_sense_reduce(handle, 0.07, nat.REDUCE_MIN, 1, scale, val, out, None, None) == nat.KB_ENOTBOUND
        assert lib.kb_sense_reduce(handle, 0.07, nat.REDUCE_MAX, 1, scale, val, out, None, None) == nat.KB_ENOTBOUND
    assert lib.kb_sense_reduce(handle, 4.0, nat.REDUCE_SUM, 8, 1.0, val, val, None, None) == nat.KB_ENOTBOUND     # in place, beyond the arena


def test_kernel_uses_no_scratch_and_spills_nothing(lib):
    """The accumulators stay in registers: every instantiation (op x row width) has a zero private segment and zero spill
    counts in the metadata of the code object that was linked."""
    found = kernel_metadata('kb_reduce_kernel')
    assert len(found) >= 1, 'no kb_reduce_kernel in the code object'
    for name, fields in found:
        for key in ('.private_segment_fixed_size', '.sgpr_spill_count', '.vgpr_spill_count'):
            assert fields[key] == 0, (name, key, fields[key])


def test_python_limits():
    for bad in (('mean', 4, 1.0), (-1, 4, 1.0), (3, 4, 1.0), ('sum', 0, 1.0), ('min', 9, 1.0), ('sum', 4, 0.0), ('sum', 4, -2.0),
                ('sum', 4, INF), ('sum', 4, NAN), (nat.REDUCE_SUM, 4, NAN)):
        with pytest.raises(ValueError):
            nat.check_reduce(*bad)
    assert nat.check_reduce('sum', 1, 65536.0) == (nat.REDUCE_SUM, 1, 65536.0)
    assert nat.check_reduce('min', 8, 1.0) == (nat.REDUCE_MIN, 8, 1.0)
    assert nat.check_reduce(nat.REDUCE_MAX, 3, 1000) == (nat.REDUCE_MAX, 3, 1000.0)
    assert nat.check_reduce('max', 2, NAN)[:2] == (nat.REDUCE_MAX, 2)       # the scale is the sum's only


def test_key_is_the_total_order_of_the_bit_patterns():
    den = np.float32(1e-45)
    v = np.array([-INF, -1e30, -1.0, -den, -0.0, 0.0, den, 1.0, INF], dtype=np.float32)
    assert den > 0 and np.signbit(v[4]) and not np.signbit(v[5])
    k = ref.key(v)
    assert k.dtype == np.uint32 and (k[1:] > k[:-1]).all()
    nans = np.array([0xFFC00001, 0xFF800001, 0x7F800001, 0x7FC00000, 0x7FFFFFFF], dtype=np.uint32).view(np.float32)
    kn = ref.key(nans)
    assert (kn[:2] < k[0]).all() and (kn[2:] > k[-1]).all()       # sign bit set: below -inf; clear: above +inf
    both = np.concatenate([v, nans])
    assert np.array_equal(ref.bits(ref.unkey(ref.key(both))), ref.bits(both))
    assert ref.key(np.float32(0.0)) == 0x80000000 and ref.key(np.float32(-0.0)) == 0x7FFFFFFF


def test_quantisation():
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 0.49999997, NAN, -NAN, INF, -INF, 3e38, -3e38, 2.0 ** 21 + 1, 1e-45, -0.0], dtype=np.float32)
    assert ref.quant(v, 1.0).tolist() == [0, 2, 2, 0, -2, 0, 0, 0, 2 ** 21, -2 ** 21, 2 ** 21, -2 ** 21, 2 ** 21, 0, 0]
    assert ref.quant(np.float32(3e38), 65536.0) == 2 ** 21 and ref.quant(np.float32(1.0), 65536.0) == 65536
    assert 1023 * 2 ** 21 < 2 ** 31


def cloud(N, seed):
    xy, _ = scenes.gaussian_spawn(1, N, sigma=0.2, seed=seed)
    return tuple((xy[0, :, k] * 25.0).astype(np.float32) for k in (0, 1))


def test_sum_is_within_the_quantisation_bound():
    """Against the float64 sum of the same messages: half a quantum per message heard plus the two final roundings (the
    int -> float conversion and the division, 2^-24 relative each)."""
    N, R, scale = 200, 0.3, 65536.0
    x, y = cloud(N, 21)
    values = np.random.RandomState(7).uniform(-1.0, 1.0, size=(N, 4)).astype(np.float32)
    out, count = ref.restate_env(x, y, values, R, 'sum', scale)
    inr = ref.in_range(x, y, R)
    exact = inr.astype(np.float64) @ values.astype(np.float64)
    err = np.abs(out.astype(np.float64) - exact)
    bound = count[:, None] * 0.5 / scale + np.abs(exact) * 2.0 ** -23
    print('pairs in range %d, at most %d heard, largest error %.3g, smallest margin %.3g' % (inr.sum(), count.max(), err.max(), (bound - err).min()))
    assert inr.sum() > 10000 and np.array_equal(count, inr.sum(1))
    assert (err <= bound).all()
    assert err.max() > 0        # (the messages are not multiples of the quantum: the bound is not met trivially)


@pytest.mark.parametrize('op', ['sum', 'min', 'max'])
def test_permuting_the_kilobots_permutes_the_result(op):
    N, R = 200, 0.3
    x, y = cloud(N, 21)
    values = np.random.RandomState(8).uniform(-1.0, 1.0, size=(N, 4)).astype(np.float32)
    out, count = ref.restate_env(x, y, values, R, op)
    perm = np.random.RandomState(9).permutation(N)
    out_p, count_p = ref.restate_env(x[perm], y[perm], values[perm], R, op)
    assert np.array_equal(ref.bits(out_p), ref.bits(out[perm])) and np.array_equal(count_p, count[perm])
    assert count.max() > 100 and len(np.unique(ref.bits(out))) > 10      # (large neighbourhoods: a min or max has few distinct values)


@pytest.mark.parametrize('N,seed,R', [(200, 21, 0.1), (333, 4, 0.05)])
def test_hop_count_is_a_breadth_first_search(N, seed, R):
    """h <- min(h, reduce_min(h) + 1) from h[0] = 0, all others +inf, until nothing changes: the identity +inf of an empty
    neighbourhood needs no special case, and kilobots out of reach stay +inf."""
    x, y = cloud(N, seed)
    want = ref.breadth_first(ref.in_range(x, y, R))
    h = np.full(N, np.inf, dtype=np.float32)
    h[0] = 0
    sweeps = 0
    while True:
        heard, _ = ref.restate_env(x, y, h, R, 'min')
        new = np.minimum(h, heard + np.float32(1))
        sweeps += 1
        if np.array_equal(new, h):
            break
        h = new
        assert sweeps <= N
    reached = np.isfinite(want)
    print('N = %d: %d sweeps, %d reached, deepest hop %d' % (N, sweeps, reached.sum(), want[reached].max()))
    assert reached.sum() > 100 and (~reached).any()
    assert np.array_equal(h, want)
    assert sweeps == want[reached].max() + 1        # (the last sweep changes nothing)


def test_batched_env_comm_radius_without_a_gpu():
    import torch
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    from tests.oracle_backend import OracleBackend
    env = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3)
    env.reset()
    a = torch.zeros(3, 16, 2)
    a[..., 0] = 0.01
    assert env.step(a)[3] == {}
    assert env.comm_radius is None
    with pytest.raises(ValueError):
        env.neighbor_reduce(torch.zeros(3, 16))
    for bad in (0.0, -0.07, NAN, (0.07, 4), 'far'):
        with pytest.raises(ValueError):
            BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, comm_radius=bad)
    ok = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3, comm_radius=0.07)
    assert ok.comm_radius == 0.07
    assert torch.equal(ok.reset(), BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3).reset())
    assert ok.step(a)[3] == {}      # reset() and step() gain nothing from comm_radius
