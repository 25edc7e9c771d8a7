"""kb_field_step without a GPU: the symbol is exported, bound and declared, the host-side validation answers in the header's
order (arguments before the bound check, so none of it needs a device), the kernel's instantiations have no private segment
and no spill (the code object's metadata), and the numpy restatement (tests/field_ref.py) has the properties the definition
is meant to have, exactly: a uniform plane is a fixed point, diffusion with keep = 1 conserves a dyadic mass, mirror images
stay mirror images, k iterations are k calls, and the deposit is the fixed-point sum.  BatchedKilobotsEnv runs its field
logic on the oracle backend with the restatement in the place of the kernel."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from tests import field_ref as ref
from tests.host_common import abi_mismatches, Handle, lib, prototypes, tab  # noqa: F401
from tests.sensing_common import kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_symbol_is_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, 'include', 'kilobots_hip.h')).read()
    assert re.search(r'\bint\s+kb_field_step\s*\(', hdr)
    assert 'kb_field_step' in nat.EXPORTS and hasattr(lib, 'kb_field_step')
    assert lib.kb_field_step.argtypes is not None and len(lib.kb_field_step.argtypes) == 12
    assert set(re.findall(r'\b(kb_[a-z_]+)\s*\(', hdr)) == set(nat.EXPORTS)
    ret, params = prototypes()['kb_field_step']
    assert ret.strip() == 'int' and len(params) == 12
    assert abi_mismatches(nat.SIGNATURES, lambda name: (getattr(lib, name).restype, getattr(lib, name).argtypes)) == []
    for name, value in (('KB_FIELD_MAX_CHANNELS', nat.FIELD_MAX_CHANNELS), ('KB_FIELD_MAX_ITERS', nat.FIELD_MAX_ITERS)):
        assert int(re.search(r'#define\s+%s\s+(\d+)' % name, hdr).group(1)) == value
    assert (ref.MAX_CHANNELS, ref.MAX_ITERS) == (nat.FIELD_MAX_CHANNELS, nat.FIELD_MAX_ITERS)


def test_check_field():
    assert nat.check_field(64, 48, 1, 1.0, 0.0, 1) == (64, 48, 1, (1.0,), (0.0,), 1)
    assert nat.check_field(128, 1, 4, 0.5, 0.25, 64) == (128, 1, 4, (0.5,) * 4, (0.25,) * 4, 64)
    assert nat.check_field(1, 128, 2, (0.0, 1.0), [0.125, 0.0], 0) == (1, 128, 2, (0.0, 1.0), (0.125, 0.0), 0)
    assert nat.check_field(3.0, 2, 3, 1, 0, 7)[:3] == (3, 2, 3)
    nan = float('nan')
    for bad in ((0, 4, 1, 1.0, 0.0, 1), (4, 0, 1, 1.0, 0.0, 1), (129, 4, 1, 1.0, 0.0, 1), (4, 129, 1, 1.0, 0.0, 1), (True, 4, 1, 1.0, 0.0, 1),
                (4, 4, 0, 1.0, 0.0, 1), (4, 4, 5, 1.0, 0.0, 1), (4, 4, True, 1.0, 0.0, 1),
                (4, 4, 1, 1.5, 0.0, 1), (4, 4, 1, -0.1, 0.0, 1), (4, 4, 1, nan, 0.0, 1), (4, 4, 2, (1.0,), 0.0, 1), (4, 4, 2, (1.0, 2.0), 0.0, 1),
                (4, 4, 1, 1.0, 0.26, 1), (4, 4, 1, 1.0, -0.01, 1), (4, 4, 1, 1.0, nan, 1), (4, 4, 2, 1.0, (0.1, 0.1, 0.1), 1),
                (4, 4, 1, 1.0, 0.0, -1), (4, 4, 1, 1.0, 0.0, 65), (4, 4, 1, 1.0, 0.0, True), ('a', 4, 1, 1.0, 0.0, 1)):
        with pytest.raises(ValueError):
            nat.check_field(*bad)


def floats(*v):
    return (C.c_float * len(v))(*v)


def test_validation_on_an_unbound_handle(lib):
    """Nothing here launches: no device pointer is dereferenced on the host.  The errors come in the header's order, each held
    against the one after it: NULL sim, gw / gh, n_channels, keep / spread, n_iters, NULL d_field, nothing to do, a d_sense
    off 16 bytes; legal arguments reach the bound check."""
    out, odd, msk = C.c_void_p(0x1000), C.c_void_p(0x1004), C.c_void_p(0x3000)
    ok, one, nan = floats(1.0, 0.5, 0.0, 1.0), floats(0.25, 0.0, 0.125, 0.25), float('nan')
    with Handle(lib) as h:
        # (sim, gw, gh, n_channels, keep, spread, n_iters, d_env_mask, d_amount, d_field, d_sense)
        bad = [
            ('NULL sim', (None, 8, 8, 1, ok, one, 1, None, out, out, out), b'NULL handle'),
            ('NULL sim before a bad grid', (None, 0, 8, 1, ok, one, 1, None, out, out, out), b'NULL handle'),
            ('gw = 0', (h, 0, 8, 1, ok, one, 1, None, out, out, out), b'KB_GRID_MAX_SIDE'),
            ('gh too large', (h, 8, 129, 1, ok, one, 1, msk, out, out, out), b'KB_GRID_MAX_SIDE'),
            ('negative gw', (h, -3, 8, 1, ok, one, 1, None, out, out, out), b'KB_GRID_MAX_SIDE'),
            ('the grid before the channels', (h, 129, 8, 0, ok, one, 1, None, out, out, out), b'KB_GRID_MAX_SIDE'),
            ('no channel', (h, 8, 8, 0, ok, one, 1, None, out, out, out), b'KB_FIELD_MAX_CHANNELS'),
            ('too many channels', (h, 8, 8, 5, ok, one, 1, None, out, out, out), b'KB_FIELD_MAX_CHANNELS'),
            ('the channels before keep', (h, 8, 8, 5, None, one, 1, None, out, out, out), b'KB_FIELD_MAX_CHANNELS'),
            ('NULL keep', (h, 8, 8, 1, None, one, 1, None, out, out, out), b'keep and spread'),
            ('NULL spread', (h, 8, 8, 1, ok, None, 1, None, out, out, out), b'keep and spread'),
            ('keep above 1', (h, 8, 8, 2, floats(1.0, 1.5), one, 1, None, out, out, out), b'[0, 1]'),
            ('negative keep', (h, 8, 8, 1, floats(-0.25), one, 1, None, out, out, out), b'[0, 1]'),
            ('NaN keep', (h, 8, 8, 1, floats(nan), one, 1, None, out, out, out), b'[0, 1]'),
            ('spread above a quarter', (h, 8, 8, 3, ok, floats(0.0, 0.25, 0.26), 1, None, out, out, out), b'[0, 0.25]'),
            ('negative spread', (h, 8, 8, 1, ok, floats(-0.125), 1, None, out, out, out), b'[0, 0.25]'),
            ('NaN spread', (h, 8, 8, 4, ok, floats(0.0, 0.0, 0.0, nan), 1, None, out, out, out), b'[0, 0.25]'),
            ('keep before the iterations', (h, 8, 8, 1, floats(2.0), one, -1, None, out, out, out), b'[0, 1]'),
            ('negative iterations', (h, 8, 8, 1, ok, one, -1, None, out, out, out), b'KB_FIELD_MAX_ITERS'),
            ('too many iterations', (h, 8, 8, 1, ok, one, 65, None, out, out, out), b'KB_FIELD_MAX_ITERS'),
            ('the iterations before the field', (h, 8, 8, 1, ok, one, 65, None, out, None, out), b'KB_FIELD_MAX_ITERS'),
            ('NULL d_field', (h, 8, 8, 1, ok, one, 1, None, out, None, out), b'd_field is NULL'),
            ('the field before nothing to do', (h, 8, 8, 1, ok, one, 0, None, None, None, None), b'd_field is NULL'),
            ('nothing to do', (h, 8, 8, 1, ok, one, 0, None, None, out, None), b'nothing to do'),
            ('nothing to do, with a mask', (h, 128, 128, 4, ok, one, 0, msk, None, odd, None), b'nothing to do'),
            ('d_sense off 16 bytes', (h, 8, 8, 1, ok, one, 1, None, out, out, odd), b'16-byte'),
            ('d_sense alone off 16 bytes', (h, 1, 1, 1, ok, one, 0, None, None, out, C.c_void_p(0x1008)), b'16-byte'),
        ]
        for what, args, word in bad:
            lib.kb_sense_neighbors(None, 0.07, 8, out, out, out, None)     # (leaves a message that the next call must replace)
            assert lib.kb_field_step(*args, None) == nat.KB_EINVAL, what
            msg = lib.kb_last_error()
            assert msg and b'kb_field_step' in msg and word in msg, (what, msg)
        # legal arguments reach the bound check: the limits themselves, a field that is only float aligned, each job alone
        for args in ((8, 8, 1, ok, one, 1, None, out, out, out), (128, 128, 4, ok, one, 64, msk, out, odd, out), (1, 1, 1, ok, one, 0, None, out, odd, None),
                     (127, 95, 3, ok, one, 0, None, None, odd, out), (64, 48, 2, floats(0.0, 1.0), floats(0.0, 0.25), 1, msk, None, out, None)):
            assert lib.kb_field_step(h, *args, None) == nat.KB_ENOTBOUND, args
            assert b'kb_field_step' in lib.kb_last_error() and b'kb_bind' in lib.kb_last_error()


def test_kernel_uses_no_scratch_and_spills_nothing(lib):
    """The cells of a lane are register arrays indexed by constants: a zero private segment and zero spill counts in the
    metadata of every instantiation (cells per lane x vector or scalar path) of the code object that was linked."""
    found = kernel_metadata('kb_field_kernel')
    assert len(found) == 10, found
    for name, fields in found:
        for key in ('.private_segment_fixed_size', '.sgpr_spill_count', '.vgpr_spill_count'):
            assert fields[key] == 0, (name, key, fields[key])


# ---- the restatement, exactly ----------------------------------------------------------------------------------------------
def run(F, keep, spread, iters):
    return ref.plane_step(F, None, None, f32(keep), f32(spread), iters)[0]


def test_a_uniform_plane_is_a_fixed_point():
    for value in (1.0, 0.1, 3.0e-5, 12345.678):
        F = np.full((11, 9), value, dtype=np.float32)
        for spread in (0.0, 0.1, 0.25):
            for iters in (1, 2, 7, 64):
                assert np.array_equal(ref.bits(run(F, 1.0, spread, iters)), ref.bits(F)), (value, spread, iters)


def test_one_deposit_spreads_symmetrically_and_keeps_its_mass():
    """1.0 at the centre of 9 x 11, keep = 1, spread = 0.25: every value stays a multiple of 2^-16 and the plane sums to
    exactly 1.0 after each of 8 iterations; it stays its own mirror image in x and in y."""
    gw, gh = 9, 11
    flat = np.array([5 * gw + 4])
    u, dep = ref.plane_step(np.zeros((gh, gw), np.float32), flat, f32([1.0]), f32(1.0), f32(0.25), 0)
    assert u[5, 4] == 1.0 and u.sum() == 1.0 and dep[flat[0]] == 1.0
    for it in range(8):
        u = ref.iterate(u, f32(1.0), f32(0.25))
        scaled = u.astype(np.float64) * 65536.0
        assert np.array_equal(scaled, np.rint(scaled)), it
        assert u.astype(np.float64).sum() == 1.0, it
        assert np.array_equal(ref.bits(u), ref.bits(u[:, ::-1])) and np.array_equal(ref.bits(u), ref.bits(u[::-1])), it
    # (spread = 0.25 is the plain average of the four neighbours: the mass hops between the two colours of the chequerboard,
    # and after 8 hops every cell of the centre's colour holds some -- all 49 are within 8 steps --, plus what the edges fold back)
    assert u[5, 4] < 1.0 and (u > 0).sum() >= 49 and (u >= 0).all()


def test_mirror_images_and_repeated_calls():
    rng = np.random.RandomState(3)
    F = rng.uniform(-2.0, 2.0, size=(7, 10)).astype(np.float32)
    for keep, spread in ((1.0, 0.25), (0.9, 0.17), (0.5, 0.0)):
        G = run(F, keep, spread, 5)
        assert np.array_equal(ref.bits(run(F[:, ::-1].copy(), keep, spread, 5)), ref.bits(G[:, ::-1]))
        assert np.array_equal(ref.bits(run(F[::-1].copy(), keep, spread, 5)), ref.bits(G[::-1]))
        u = F
        for _ in range(5):
            u = run(u, keep, spread, 1)
        assert np.array_equal(ref.bits(u), ref.bits(G))


def test_deposit_is_the_fixed_point_sum(tab):
    acc, dep = ref.deposit(np.zeros(1024, dtype=np.int64), ref.quant(np.full(1024, 16.0, np.float32)), 4)
    assert acc[0] == 2 ** 30 and dep[0] == 16384.0 and not acc[1:].any()
    assert ref.quant(f32([16.0, 17.0, -1e9, np.inf, -np.inf])).tolist() == [2 ** 20, 2 ** 20, -2 ** 20, 2 ** 20, -2 ** 20]
    assert ref.quant(f32([np.nan, 1.5 / 65536, 2.5 / 65536, -0.5 / 65536, 1.0])).tolist() == [0, 2, 2, 0, 65536]
    nan = ref.deposit(np.array([2, 2, 3]), ref.quant(f32([np.nan, 0.5, np.nan])), 4)
    assert nan[0].tolist() == [0, 0, 32768, 0] and nan[1].tolist() == [0.0, 0.0, 0.5, 0.0]
    # the order of the kilobots is nothing to the sum; without amounts the bits of the plane pass through
    rng = np.random.RandomState(5)
    E, N, C_, gw, gh = 2, 50, 2, 7, 5
    x, y = rng.uniform(-26, 26, (E, N)).astype(np.float32), rng.uniform(-20, 20, (E, N)).astype(np.float32)
    th, am = rng.uniform(-3, 3, (E, N)).astype(np.float32), rng.uniform(-2, 2, (E, N, C_)).astype(np.float32)
    F = rng.uniform(-1, 1, (E, C_, gh, gw)).astype(np.float32)
    F[0, 0, 0, 0] = -0.0
    G, rows = ref.restate(tab, F, x, y, th, am, (1.0, 0.9), (0.25, 0.1), 3)
    p = rng.permutation(N)
    G2, rows2 = ref.restate(tab, F, x[:, p], y[:, p], th[:, p], am[:, p], (1.0, 0.9), (0.25, 0.1), 3)
    assert np.array_equal(ref.bits(G), ref.bits(G2)) and np.array_equal(ref.bits(rows[:, p]), ref.bits(rows2))
    G3, rows3 = ref.restate(tab, F, x, y, th, None, 1.0, 0.0, 0)
    assert np.array_equal(ref.bits(G3), ref.bits(F)) and not ref.bits(rows3[..., 3]).any()
    ix, iy = ref.grid_ref.cells(tab, gw, gh, x[0], y[0])
    assert np.array_equal(ref.bits(rows3[0, :, 1, 0]), ref.bits(F[0, 1, iy, ix]))
    masked, kept = ref.restate(tab, F, x, y, th, am, 1.0, 0.1, 1, env_mask=np.array([0, 1]), fill=np.full((E, N, C_, 4), 7, np.float32))
    assert np.array_equal(ref.bits(masked[0]), ref.bits(F[0])) and (kept[0] == 7).all() and (masked[1] != F[1]).any()


# ---- the env on the oracle backend, the restatement in the place of the kernel ----------------------------------------------
def field_backend(tab):
    import torch
    from tests.oracle_backend import OracleBackend

    class FieldBackend(OracleBackend):
        calls = []

        def new_field(self, width, height, channels=1):
            return torch.zeros(self.num_envs, channels, height, width)

        def field_step(self, field, amount=None, keep=1.0, spread=0.0, iters=1, env_mask=None, sense=True, out=None):
            width, height, channels, keep, spread, iters = nat.check_field(field.shape[3], field.shape[2], field.shape[1], keep, spread, iters)
            FieldBackend.calls.append((amount is None, iters))
            G, rows = ref.restate(tab, field.numpy(), self.x.numpy(), self.y.numpy(), self.theta.numpy(), None if amount is None else amount.numpy(),
                                  keep, spread, iters, None if env_mask is None else env_mask.numpy(), sense)
            field.copy_(torch.from_numpy(G))
            return torch.from_numpy(rows) if sense else None
    return FieldBackend


def test_batched_env_field_obs_without_a_gpu(tab):
    import torch
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    from gym_kilobots_amd.envs.batched_env import OPTIONS
    Backend = field_backend(tab)
    E, N = 3, 16
    assert 'field_obs' in OPTIONS
    plain = BatchedKilobotsEnv(E, N, sim_factory=Backend, seed=3)
    assert plain.field_obs is None and plain.field is None
    with pytest.raises(ValueError):
        plain.field_sense()
    for bad in (5, (64,), (64, 48, 1, 1), (0, 48), (64, 129), (8, 8, 0), (8, 8, 5), ('a', 'b'), (True, 8)):
        with pytest.raises(ValueError):
            BatchedKilobotsEnv(E, N, sim_factory=Backend, field_obs=bad)
    for kw in (dict(field_keep=1.5), dict(field_spread=0.3), dict(field_iters=65), dict(field_iters=-1), dict(field_keep=(1.0, 1.0))):
        with pytest.raises(ValueError):
            BatchedKilobotsEnv(E, N, sim_factory=Backend, field_obs=(8, 6), **kw)
    assert BatchedKilobotsEnv(E, N, sim_factory=Backend, field_obs=[8, 6]).field_obs == (8, 6, 1)

    seen = []

    def deposit(prev, actions, obs):
        seen.append((prev.shape, obs.shape))
        return torch.full((E, N, 2), 0.5)
    env = BatchedKilobotsEnv(E, N, sim_factory=Backend, seed=3, field_obs=(8, 6, 2), field_keep=(1.0, 0.5), field_spread=0.125, field_iters=2, deposit_fn=deposit)
    assert env.field_obs == (8, 6, 2) and tuple(env.field.shape) == (E, 2, 6, 8)
    assert torch.equal(env.reset(), plain.reset())
    a = torch.zeros(E, N, 2)
    a[..., 0] = 0.01
    Backend.calls.clear()
    obs, _, _, info = env.step(a)
    pobs, _, _, pinfo = plain.step(a)
    assert torch.equal(obs, pobs) and pinfo == {} and sorted(info) == ['field'] and Backend.calls == [(False, 2)]
    assert seen == [((E, N, 3), (E, N, 3))]
    rows = info['field']
    assert tuple(rows.shape) == (E, N, 2, 4)
    assert float(env.field[:, 0].sum()) == E * N * 0.5 and float(env.field[:, 1].sum()) == E * N * 0.5 * 0.25     # (keep = 1 conserves, 0.5 twice)
    assert (rows[..., 3].sum(1) >= 0.5 * N).all()       # every kilobot reports what its cell received, its own share included
    kept = env.field.clone()
    read = env.field_sense()
    assert torch.equal(env.field, kept) and torch.equal(read[..., :3], rows[..., :3]) and not read[..., 3].any()
    env.step(a)
    assert float(env.field[:, 0].sum()) == 2 * E * N * 0.5
    env.reset()
    assert not env.field.any()
    # without a deposit_fn every kilobot deposits 1.0 in every channel
    ones = BatchedKilobotsEnv(E, N, sim_factory=Backend, seed=3, field_obs=(8, 6, 3), field_iters=0)
    ones.reset()
    ones.step(a)
    assert (ones.field.sum((2, 3)) == N).all()
