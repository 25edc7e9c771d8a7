"""kb_sense_grid and kb_grid_channels without a GPU: the symbols are exported, bound and declared, the host-side validation
answers in the header's order (arguments before the bound check, so none of it needs a device), both kernels have no private
segment and no spill (the code object's metadata), and the numpy restatement (tests/grid_ref.py) is the intended quantity:
the count plane sums to the kilobots of the env wherever they are, the flow planes sum to the quantised headings, and the
object masks are those of the same predicate in float64.  BatchedKilobotsEnv checks grid_obs at construction."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from tests import grid_ref as ref
from tests import objects_ref
from tests import reduce_ref
from tests import scenes
from tests.host_common import Handle, lib  # noqa: F401
from tests.sensing_common import f32, kernel_metadata, wall_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(1, 1), (3, 2), (7, 5), (64, 48), (127, 95), (128, 128)]


def test_symbols_are_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, 'include', 'kilobots_hip.h')).read()
    assert re.search(r'\bint\s+kb_sense_grid\s*\(', hdr) and re.search(r'\bint\s+kb_grid_channels\s*\(', hdr)
    for name, nargs in (('kb_sense_grid', 6), ('kb_grid_channels', 2)):
        assert name in nat.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == nargs
    for name, value in (('COUNT', 1), ('FLOW', 2), ('OBJECTS', 4), ('MAX_SIDE', 128)):
        assert re.search(r'#define\s+KB_GRID_%s\s+%d\b' % (name, value), hdr) and getattr(nat, 'GRID_' + name) == value
    assert (ref.COUNT, ref.FLOW, ref.OBJECTS) == (nat.GRID_COUNT, nat.GRID_FLOW, nat.GRID_OBJECTS)


def test_check_grid():
    assert nat.check_grid(64, 48, ('count',)) == (64, 48, 1)
    assert nat.check_grid(1, 128, ['flow', 'count']) == (1, 128, 3)
    assert nat.check_grid(128, 1, ('objects', 'count', 'flow')) == (128, 1, 7)
    assert nat.check_grid(3, 2, 'flow') == (3, 2, 2) and nat.check_grid(3, 2, nat.GRID_OBJECTS | nat.GRID_COUNT) == (3, 2, 5)
    for bad in ((0, 4, 1), (4, 0, 1), (129, 4, 1), (4, 129, 1), (4, 4, 0), (4, 4, 8), (4, 4, -1), (4, 4, ()), (4, 4, ('heat',)), (4, 4, 'counts'),
                (4, 4, True)):
        with pytest.raises(ValueError):
            nat.check_grid(*bad)


def test_validation_on_an_unbound_handle(lib):
    """Nothing here launches: the pointer is never dereferenced on the host (any non-NULL value will do, float alignment
    is all the entry asks for).  The errors come in the header's order: NULL, planes, gw / gh, objects without objects."""
    out = C.c_void_p(0x1004)
    with Handle(lib) as plain, Handle(lib, num_objects=2) as two:
        bad = [
            ('NULL sim', (None, 8, 8, 1, out), b'NULL'),
            ('NULL d_out', (two, 8, 8, 1, None), b'NULL'),
            ('NULL d_out before bad planes', (two, 8, 8, 0, None), b'NULL'),
            ('no plane', (two, 8, 8, 0, out), b'planes'),
            ('an unknown plane', (two, 8, 8, 8, out), b'planes'),
            ('negative planes', (two, 8, 8, -1, out), b'planes'),
            ('planes before the grid', (two, 0, 8, 16, out), b'planes'),
            ('gw = 0', (two, 0, 8, 7, out), b'KB_GRID_MAX_SIDE'),
            ('gh = 0', (two, 8, 0, 7, out), b'KB_GRID_MAX_SIDE'),
            ('gw too large', (two, 129, 8, 7, out), b'KB_GRID_MAX_SIDE'),
            ('gh too large', (two, 8, 129, 1, out), b'KB_GRID_MAX_SIDE'),
            ('the grid before the objects', (plain, 129, 8, 4, out), b'KB_GRID_MAX_SIDE'),
            ('objects without objects', (plain, 8, 8, 4, out), b'no objects'),
            ('all planes without objects', (plain, 128, 128, 7, out), b'no objects'),
        ]
        for what, args, word in bad:
            lib.kb_sense_neighbors(None, 0.07, 8, out, out, out, None)     # (leaves a message that the next call must replace)
            assert lib.kb_sense_grid(*args, None) == nat.KB_EINVAL, what
            msg = lib.kb_last_error()
            assert msg and b'kb_sense_grid' in msg and word in msg, (what, msg)
        # legal arguments reach the bound check
        for h, args in ((two, (8, 8, 7)), (two, (128, 128, 4)), (two, (1, 1, 2)), (plain, (127, 95, 3)), (plain, (64, 48, 1))):
            assert lib.kb_sense_grid(h, *args, out, None) == nat.KB_ENOTBOUND
            assert b'kb_sense_grid' in lib.kb_last_error() and b'kb_bind' in lib.kb_last_error()
        # kb_grid_channels needs neither buffers nor a device
        assert [lib.kb_grid_channels(two, p) for p in range(1, 8)] == [1, 2, 3, 2, 3, 4, 5]
        assert [lib.kb_grid_channels(plain, p) for p in (1, 2, 3)] == [1, 2, 3]
        for h, p in ((None, 1), (two, 0), (two, 8), (two, -1), (plain, 4), (plain, 7)):
            lib.kb_sense_neighbors(None, 0.07, 8, out, out, out, None)
            assert lib.kb_grid_channels(h, p) == nat.KB_EINVAL and b'kb_grid_channels' in lib.kb_last_error()


def test_kernels_use_no_scratch_and_spill_nothing(lib):
    """The counters live in LDS and the object walk in scalars: every instantiation of the two kernels has a zero private
    segment and zero spill counts in the metadata of the code object that was linked."""
    found = kernel_metadata('grid')
    names = [n for n, _ in found]
    assert any('kb_grid_bots_kernel' in n for n in names) and any('kb_grid_objects_kernel' in n for n in names), names
    assert len([n for n in names if 'kb_grid_bots_kernel' in n]) == 3       # count, flow, count + flow
    for name, fields in found:
        for key in ('.private_segment_fixed_size', '.sgpr_spill_count', '.vgpr_spill_count'):
            assert fields[key] == 0, (name, key, fields[key])


def world(xy_m):
    xy = np.asarray(xy_m, np.float64) * 25.0        # (KilobotSim.set_poses_m)
    return f32(xy[..., 0]), f32(xy[..., 1])


@pytest.fixture(scope='module')
def plain_tab(lib):
    with Handle(lib) as h:
        return objects_ref.tables(nat.outline(h))


@pytest.mark.parametrize('scene', ['gaussian', 'walls'])
def test_restated_kilobot_planes_are_the_intended_sums(plain_tab, scene):
    """On a Gaussian spawn and on the wall scene, whose kilobots lie partly outside the arena: every kilobot is counted
    exactly once, in a cell of the grid, and the flow planes hold nothing but the quantised headings."""
    if scene == 'gaussian':
        xy, th = scenes.gaussian_spawn(3, 333, sigma=0.3, seed=12)
    else:
        xy, th = wall_scene(random_headings=True)
    x, y = world(xy)
    th = f32(th)
    E, N = x.shape
    ar = plain_tab['arena']
    outside = (x < ar[0]) | (x > ar[1]) | (y < ar[2]) | (y > ar[3])
    assert outside.any() == (scene == 'walls')
    for gw, gh in GRIDS:
        g = ref.restate(plain_tab, gw, gh, ref.COUNT | ref.FLOW, x, y, th)
        assert g.dtype == np.float32 and g.shape == (E, 3, gh, gw)
        for e in range(E):
            assert g[e, 0].sum(dtype=np.float64) == N and (g[e, 0] == np.rint(g[e, 0])).all() and (g[e, 0] >= 0).all()
            qc, qs = ref.quantised_headings(th[e])
            # (multiples of 2^-16 below 2^10: float64 sums of them are exact)
            assert g[e, 1].sum(dtype=np.float64) == qc.sum(dtype=np.int64) / 65536.0
            assert g[e, 2].sum(dtype=np.float64) == qs.sum(dtype=np.int64) / 65536.0
            assert np.array_equal(qc, reduce_ref.quant(f32([objects_ref.O.sincosf(float(t))[1] for t in th[e]]), 65536.0))
            # where nobody is, the flow is +0.0; a lone kilobot's cell holds its own quantised heading
            empty = g[e, 0] == 0
            assert not ref.bits(g[e, 1:][:, empty]).any()
            ix, iy = ref.cells(plain_tab, gw, gh, x[e], y[e])
            assert ((0 <= ix) & (ix < gw) & (0 <= iy) & (iy < gh)).all()
            lone = np.flatnonzero(g[e, 0][iy, ix] == 1)
            assert np.array_equal(g[e, 1][iy[lone], ix[lone]], f32(qc[lone]) / f32(65536))
        if gw >= 64:
            # inside the arena the cell is the one whose bounds hold the kilobot, up to the rounding of one cell index
            ix, iy = ref.cells(plain_tab, gw, gh, x[0], y[0])
            fx = (x[0].astype(np.float64) - float(ar[0])) / (float(ar[1]) - float(ar[0])) * gw
            assert (np.abs(ix - np.clip(np.floor(fx), 0, gw - 1)) <= 1).all() and (ix == np.clip(np.floor(fx), 0, gw - 1)).mean() > 0.99


@pytest.mark.parametrize('name', ['disc', 'boxes', 'mixed', 'forms'])
def test_restated_object_masks_equal_the_float64_evaluation(lib, name):
    """The masks of the float32 restatement against the same predicate in float64 on the same cell centres: they may differ
    only at cells whose float64 distance to the outline is below the rounding bound that tests/test_objects_cpu.py derives
    (1.95e-5 m).  A band that narrow around every outline holds about one cell centre in ten per object at 128 x 128, so
    the seed of the object poses was chosen, on the float64 evaluation alone, as one that leaves no centre inside it
    (the nearest is 2.96e-5 m away): the masks are then equal.  From 64 x 48 upward every object covers several cell
    centres, and never most of them."""
    kw, centres = objects_ref.object_sets()[name]
    with Handle(lib, **kw) as h:
        tab = objects_ref.tables(nat.outline(h))
    _, _, objs, oth = objects_ref.spawn_over_objects(1, 1, centres, seed=55)
    ox, oy = world(objs[0])
    oth = f32(oth[0])
    for gw, gh in ((64, 48), (127, 95), (128, 128)):
        m32, _ = ref.object_masks(tab, gw, gh, ox, oy, oth)
        m64, d64 = ref.object_masks(tab, gw, gh, ox, oy, oth, ft=np.float64)
        assert m32.dtype == np.float32 and m32.shape == (tab['M'], gh, gw) and set(np.unique(m32)) == {0.0, 1.0}
        near = d64 < objects_ref.BOUND_M
        print('%s %d x %d: %d cells within the bound of an outline, %d cells differ, cells covered per object %s'
              % (name, gw, gh, near.sum(), (m32 != m64).sum(), m32.sum((1, 2)).astype(int).tolist()))
        assert not (m32 != m64)[~near].any()
        assert not near.any()
        assert np.array_equal(m32, m64.astype(np.float32))
        assert (m32.sum((1, 2)) >= 4).all() and (m32.sum((1, 2)) < gw * gh / 4).all()      # (the smallest, a disc of 0.04 m, has the area of 5.1 cells at 64 x 48)
        full = ref.restate_env(tab, gw, gh, ref.ALL, f32([0.0]), f32([0.0]), f32([0.0]), ox, oy, oth)
        assert full.shape == (3 + tab['M'], gh, gw) and np.array_equal(full[3:], m32)


def test_batched_env_grid_obs_without_a_gpu():
    import torch
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    from tests.oracle_backend import OracleBackend
    env = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3)
    env.reset()
    a = torch.zeros(3, 16, 2)
    a[..., 0] = 0.01
    assert env.step(a)[3] == {} and env.grid_obs is None
    with pytest.raises(ValueError):
        env.occupancy_grid()
    for bad in (5, (64,), (64, 48, 1, 2), (0, 48), (64, 129), (64, 48, ()), (64, 48, ('heat',)), (64, 48, 8), (64, 48, ('objects',)),
                (64, 48, ('count', 'objects')), (64, 48, 7), ('a', 'b')):
        with pytest.raises(ValueError):
            BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, grid_obs=bad)
    ok = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3, grid_obs=(64, 48))
    assert ok.grid_obs == (64, 48, nat.GRID_COUNT)
    assert torch.equal(ok.reset(), BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3).reset())
    assert BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, grid_obs=[32, 24, ('flow', 'count')]).grid_obs == (32, 24, 3)
