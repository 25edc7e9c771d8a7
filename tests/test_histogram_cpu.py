"""kb_sense_histogram / kb_histogram_sectors without a GPU: the symbols are exported and bound, the sector table is what the
header says, the host-side validation answers in the header's order (arguments before the bound check, so none of it
needs a device), the kernel keeps its counters out of private memory (no scratch, no spills in the code object's
metadata), and BatchedKilobotsEnv checks histogram_obs at construction."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from tests import histogram_ref as ref
from tests import scenes
from tests.host_common import handle, lib  # noqa: F401
from tests.sensing_common import kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, 'include', 'kilobots_hip.h')).read()
    for name, nargs in (('kb_sense_histogram', 7), ('kb_histogram_sectors', 2)):
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), name
        assert name in nat.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == nargs
    assert set(re.findall(r'\b(kb_[a-z_]+)\s*\(', hdr)) == set(nat.EXPORTS)
    for define, value in (('KB_HIST_MAX_RINGS', nat.HIST_MAX_RINGS), ('KB_HIST_MAX_SECTORS', nat.HIST_MAX_SECTORS),
                          ('KB_HIST_MAX_BINS', nat.HIST_MAX_BINS)):
        m = re.search(r'#define\s+' + define + r'\s+(\d+)', hdr)
        assert m and int(m.group(1)) == value, define
    assert (nat.HIST_MAX_RINGS, nat.HIST_MAX_SECTORS, nat.HIST_MAX_BINS) == (8, 16, 64)


@pytest.mark.parametrize('n', [2, 4, 6, 8, 10, 12, 14, 16])
def test_sector_table(lib, n):
    H = n // 2
    rows = H - 1
    buf = (C.c_float * (2 * rows + 2))(*([7.0] * (2 * rows + 2)))
    assert lib.kb_histogram_sectors(n, buf) == 0
    assert buf[2 * rows] == 7.0 and buf[2 * rows + 1] == 7.0          # n / 2 - 1 rows, nothing behind them
    u = np.array(buf[:2 * rows], dtype=np.float32).reshape(rows, 2)
    assert len(nat.histogram_sectors(n)) == rows
    for m in range(1, H):
        assert abs(float(u[m - 1, 0]) - math.cos(math.pi * m / H)) <= 1e-7
        assert abs(float(u[m - 1, 1]) - math.sin(math.pi * m / H)) <= 1e-7
        if 2 * m == H:
            assert u[m - 1, 0] == 0.0 and u[m - 1, 1] == 1.0 and not np.signbit(u[m - 1, 0])
    # strictly counter-clockwise: from dead ahead (1, 0) through the rows to dead astern (-1, 0)
    if rows:        # (n = 2 has no boundary between dead ahead and dead astern)
        ring = np.vstack([[1.0, 0.0], u.astype(np.float64), [-1.0, 0.0]])
        assert (ring[:-1, 0] * ring[1:, 1] - ring[:-1, 1] * ring[1:, 0] > 0).all()
    assert (u[:, 1] > 0).all()


def test_sector_table_limits(lib):
    buf = (C.c_float * 4)(7.0, 7.0, 7.0, 7.0)
    for n in (1, 2):                # empty tables: nothing written, NULL allowed
        assert lib.kb_histogram_sectors(n, buf) == 0
        assert list(buf) == [7.0] * 4
        assert lib.kb_histogram_sectors(n, None) == 0
    for n in (0, 3, 18, -2, 17):
        lib.kb_histogram_sectors(4, None)
        assert lib.kb_histogram_sectors(n, buf) == nat.KB_EINVAL, n
        assert b'kb_histogram_sectors' in lib.kb_last_error()
    assert lib.kb_histogram_sectors(4, None) == nat.KB_EINVAL
    assert b'kb_histogram_sectors' in lib.kb_last_error()
    with pytest.raises(nat.KilobotsHipError):
        nat.histogram_sectors(3)


def test_validation_on_an_unbound_handle(lib, handle):
    """Nothing here launches: the pointers are never dereferenced on the host (any non-NULL value will do)."""
    hist, cnt = C.c_void_p(0x1000), C.c_void_p(0x2000)
    bad = [
        ('rings = 0', (handle, 0.07, 0, 8, hist, cnt, None)),
        ('rings = 9', (handle, 0.07, 9, 4, hist, cnt, None)),
        ('sectors = 0', (handle, 0.07, 4, 0, hist, cnt, None)),
        ('sectors = 3', (handle, 0.07, 4, 3, hist, cnt, None)),
        ('sectors = 18', (handle, 0.07, 2, 18, hist, cnt, None)),
        ('8 x 16 bins', (handle, 0.07, 8, 16, hist, cnt, None)),
        ('radius = 0', (handle, 0.0, 4, 8, hist, cnt, None)),
        ('radius = -1', (handle, -1.0, 4, 8, hist, cnt, None)),
        ('radius = NaN', (handle, float('nan'), 4, 8, hist, cnt, None)),
        ('NULL d_hist', (handle, 0.07, 4, 8, None, cnt, None)),
        ('NULL sim', (None, 0.07, 4, 8, hist, cnt, None)),
    ]
    for what, args in bad:
        lib.kb_sense_neighbors(None, 0.07, 8, hist, hist, cnt, None)     # (leaves a message that the next call must replace)
        assert lib.kb_sense_histogram(*args) == nat.KB_EINVAL, what
        msg = lib.kb_last_error()
        assert msg and b'kb_sense_histogram' in msg, what
    for rings, sectors in ((1, 1), (4, 8), (8, 8), (4, 16), (5, 1), (1, 2)):
        for c in (cnt, None):       # d_count is optional
            assert lib.kb_sense_histogram(handle, 0.07, rings, sectors, hist, c, None) == nat.KB_ENOTBOUND
            assert b'kb_sense_histogram' in lib.kb_last_error() and b'kb_bind' in lib.kb_last_error()


def test_argument_errors_come_before_the_bound_check(lib, handle):
    hist = C.c_void_p(0x1000)
    assert lib.kb_sense_histogram(handle, 0.07, 9, 8, hist, None, None) == nat.KB_EINVAL
    assert lib.kb_sense_histogram(handle, 0.07, 4, 3, hist, None, None) == nat.KB_EINVAL
    assert lib.kb_sense_histogram(handle, 0.07, 8, 16, hist, None, None) == nat.KB_EINVAL
    assert lib.kb_sense_histogram(handle, float('nan'), 4, 8, hist, None, None) == nat.KB_EINVAL
    assert lib.kb_sense_histogram(handle, 0.07, 4, 8, None, None, None) == nat.KB_EINVAL
    assert lib.kb_sense_histogram(handle, 0.07, 4, 8, hist, None, None) == nat.KB_ENOTBOUND


def test_kernel_uses_no_scratch_and_spills_nothing(lib):
    """The counters live in LDS columns, never in a per-lane array: every instantiation of the histogram kernel has a zero
    private segment and zero spill counts in the metadata of the code object that was linked (the assembly build() keeps
    next to the object)."""
    seen = 0
    for name, fields in kernel_metadata('kb_histogram_kernel'):
        seen += 1
        for key in ('.private_segment_fixed_size', '.sgpr_spill_count', '.vgpr_spill_count'):
            assert fields[key] == 0, (name, key, fields[key])
    assert seen >= 1, 'no kb_histogram_kernel in the code object'


def test_python_limits():
    for rings, sectors in ((0, 8), (9, 4), (4, 0), (4, 3), (2, 18), (8, 16), (4, -2)):
        with pytest.raises(ValueError):
            nat.check_histogram_grid(rings, sectors)
    for grid in ((1, 1), (1, 2), (5, 1), (3, 6), (4, 8), (8, 8), (4, 16)):
        assert nat.check_histogram_grid(*grid) == grid


@pytest.mark.parametrize('rings,sectors', [(4, 8), (3, 6), (4, 16), (5, 1), (1, 2)])
def test_restatement_is_the_intended_observation(lib, rings, sectors):
    """The counted comparisons of the definition bin like atan2 / sqrt in double on a Gaussian cloud, rows sum to the
    in-range count and every bin of the grid is hit: the comparisons only settle the boundary cases."""
    N, R = 200, 0.3
    xy, th = scenes.gaussian_spawn(1, N, sigma=0.2, seed=21)
    x, y = ((xy[0, :, k] * 25.0).astype(np.float32) for k in (0, 1))
    t = th[0].astype(np.float32)
    v = ref.restate_env(x, y, t, R, rings, sectors)
    assert np.array_equal(v['hist'].sum((1, 2)), v['count'].astype(np.float32))
    assert (v['hist'].sum(0) > 0).all()
    X, Y, T = x.astype(np.float64), y.astype(np.float64), t.astype(np.float64)
    ex, ey = X[None, :] - X[:, None], Y[None, :] - Y[:, None]
    dist = np.sqrt(ex * ex + ey * ey)
    Rw = float(np.float32(R) * np.float32(25))
    want_ring = np.minimum(np.ceil(dist / (Rw / rings)) - 1, rings - 1).clip(0).astype(np.int64)
    bearing = np.mod(np.arctan2(ey, ex) - T[:, None], 2 * np.pi)
    want_sector = np.floor(bearing / (2 * np.pi / sectors)).astype(np.int64) % sectors
    inr = v['inr']
    assert inr.sum() > 10000
    assert np.array_equal(v['ring'][inr], want_ring[inr])
    assert np.array_equal(v['sector'][inr], want_sector[inr])


def test_batched_env_histogram_obs_without_a_gpu():
    import torch
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    from tests.oracle_backend import OracleBackend
    env = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3, histogram_obs=None)
    env.reset()
    a = torch.zeros(3, 16, 2)
    a[..., 0] = 0.01
    assert env.step(a)[3] == {}
    assert env.histogram_obs is None
    with pytest.raises(ValueError):
        env.neighbor_histogram()
    for bad in ((0.07, 4), (0.07, 4, 8, 1), (0.0, 4, 8), (-1.0, 4, 8), (float('nan'), 4, 8), (0.07, 0, 8), (0.07, 9, 4), (0.07, 4, 3),
                (0.07, 4, 18), (0.07, 8, 16), 0.07):
        with pytest.raises(ValueError):
            BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, histogram_obs=bad)
    ok = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, histogram_obs=(0.07, 4, 8), neighbor_obs=(0.07, 8))
    assert ok.histogram_obs == (0.07, 4, 8) and ok.neighbor_obs == (0.07, 8)
