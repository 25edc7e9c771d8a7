"""kb_sense_paths and kb_path_costs without a GPU: both symbols are exported, bound and declared, the host-side validation
answers in the header's order (arguments before the bound check, so none of it needs a device), kb_path_costs equals the
restatement, the kernel has no private segment and no spill (the code object's metadata), and the restatement
(tests/paths_ref.py: Dijkstra on Python ints) is the intended quantity: D satisfies the Bellman equation over the allowed
moves, sources are 0, next is the lowest direction of descent, and with clear_m == 0 the object part of the blocked plane is
the OR of the object planes of kb_sense_grid.  The scenes of the GPU tests hold what they are there for, checked here on the
restatement alone.  nat.path_cells is the grid's cell rule, and BatchedKilobotsEnv checks path_obs at construction."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from tests import grid_ref
from tests import objects_ref
from tests import paths_ref as ref
from tests.host_common import abi_mismatches, Handle, lib, prototypes, tab  # noqa: F401
from tests.sensing_common import kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_symbols_are_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, 'include', 'kilobots_hip.h')).read()
    for name, nargs in (('kb_sense_paths', 12), ('kb_path_costs', 4)):
        assert re.search(r'\bint\s+%s\s*\(' % name, hdr)
        assert name in nat.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == nargs
        ret, params = prototypes()[name]
        assert ret.strip() == 'int' and len(params) == nargs
    assert 'kb_sense_paths' in nat.OPTIONAL
    assert set(re.findall(r'\b(kb_[a-z_]+)\s*\(', hdr)) == set(nat.EXPORTS)
    assert abi_mismatches(nat.SIGNATURES, lambda name: (getattr(lib, name).restype, getattr(lib, name).argtypes)) == []


def test_validation_on_an_unbound_handle(lib):
    """Nothing here launches: no pointer is dereferenced on the host.  The errors come in the header's order: NULL sim or
    d_source, gw / gh, objects, clear_m, all outputs NULL, a d_bot off 16 bytes; legal arguments reach the bound check."""
    out, odd, src, blk = C.c_void_p(0x1000), C.c_void_p(0x1004), C.c_void_p(0x3000), C.c_void_p(0x5001)
    nan, inf = float('nan'), float('inf')
    kw, _ = objects_ref.object_sets()['boxes']      # four objects: masks 0 .. 15
    with Handle(lib, **kw) as h, Handle(lib) as h0:
        bad = [
            ('NULL sim', (None, 8, 8, src, None, 0, 0.0, out, out, out, out), b'NULL argument'),
            ('NULL sim before a bad grid', (None, 0, 8, src, None, 0, 0.0, out, out, out, out), b'NULL argument'),
            ('NULL d_source', (h, 8, 8, None, None, 0, 0.0, out, out, out, out), b'NULL argument'),
            ('NULL d_source before a bad grid', (h, 8, 129, None, blk, 99, nan, None, None, None, None), b'NULL argument'),
            ('gw = 0', (h, 0, 8, src, None, 0, 0.0, out, out, out, out), b'KB_GRID_MAX_SIDE'),
            ('gh = 0', (h, 8, 0, src, None, 0, 0.0, out, out, out, out), b'KB_GRID_MAX_SIDE'),
            ('gw too large', (h, 129, 8, src, blk, 0, 0.0, out, None, None, None), b'KB_GRID_MAX_SIDE'),
            ('negative gh', (h, 8, -2, src, None, 0, 0.0, out, out, out, out), b'KB_GRID_MAX_SIDE'),
            ('the grid before objects', (h, 8, 129, src, None, 16, 0.0, out, out, out, out), b'KB_GRID_MAX_SIDE'),
            ('objects = 2^num_objects', (h, 8, 8, src, None, 16, 0.0, out, out, out, out), b'objects'),
            ('negative objects', (h, 8, 8, src, None, -1, 0.0, out, out, out, out), b'objects'),
            ('objects on a handle without any', (h0, 8, 8, src, None, 1, 0.0, out, out, out, out), b'objects'),
            ('objects before clear_m', (h, 8, 8, src, None, 16, -1.0, out, out, out, out), b'objects'),
            ('negative clear_m', (h, 8, 8, src, None, 15, -0.01, out, out, out, out), b'clear_m'),
            ('NaN clear_m', (h, 8, 8, src, None, 0, nan, out, out, out, out), b'clear_m'),
            ('infinite clear_m', (h, 8, 8, src, blk, 3, inf, out, out, out, out), b'clear_m'),
            ('clear_m before no output', (h, 8, 8, src, None, 0, nan, None, None, None, None), b'clear_m'),
            ('no output', (h, 8, 8, src, None, 0, 0.0, None, None, None, None), b'all NULL'),
            ('no output before the alignment', (h, 128, 128, src, blk, 15, 0.0165, None, None, None, None), b'all NULL'),
            ('d_bot off 16 bytes', (h, 8, 8, src, None, 0, 0.0, out, out, odd, out), b'16-byte'),
            ('d_bot alone off 16 bytes', (h, 1, 1, src, blk, 1, 0.5, None, None, C.c_void_p(0x1008), None), b'16-byte'),
        ]
        for what, args, word in bad:
            lib.kb_sense_neighbors(None, 0.07, 8, out, out, out, None)     # (leaves a message that the next call must replace)
            assert lib.kb_sense_paths(*args, None) == nat.KB_EINVAL, what
            msg = lib.kb_last_error()
            assert msg and b'kb_sense_paths' in msg and word in msg, (what, msg)
        # legal arguments reach the bound check: each output alone (the others byte aligned at the most), all, every mask
        for args in ((8, 8, src, None, 0, 0.0, out, out, out, out), (128, 128, src, blk, 15, 0.0165, odd, blk, out, odd),
                     (1, 1, src, None, 1, 0.0, odd, None, None, None), (127, 95, blk, None, 8, 2.0, None, blk, None, None),
                     (64, 48, src, blk, 7, 0.0, None, None, out, None), (3, 2, src, None, 0, 0.5, None, None, None, odd)):
            assert lib.kb_sense_paths(h, *args, None) == nat.KB_ENOTBOUND, args
            assert b'kb_sense_paths' in lib.kb_last_error() and b'kb_bind' in lib.kb_last_error()
        assert lib.kb_sense_paths(h0, 8, 8, src, None, 0, 0.0, out, None, None, None, None) == nat.KB_ENOTBOUND


def path_costs(lib, h, gw, gh):
    q = (C.c_int32 * 3)(-7, -7, -7)
    assert lib.kb_path_costs(h, gw, gh, q) == nat.KB_OK, lib.kb_last_error()
    return tuple(q)


def test_path_costs_equal_the_restatement(lib):
    """Square cells (64 x 48 on 2 x 1.5 m), non-square ones, one cell, the largest grid; an arena so small that every cost
    clamps to 1 and one so large that a single cell clamps to 65536.  Host only: the handles are never bound."""
    seen = set()
    for kw, grids in ((dict(), [(64, 48), (7, 5), (1, 1), (128, 128), (1, 7), (5, 1), (33, 31), (128, 96)]),
                      (dict(world_width=3.0, world_height=1.0), [(7, 5), (30, 10)]),
                      (dict(world_width=0.004, world_height=0.003), [(128, 128)]),
                      (dict(world_width=8.0, world_height=6.0), [(1, 1), (2, 1)])):
        with Handle(lib, **kw) as h:
            t = objects_ref.tables(nat.outline(h))
            for gw, gh in grids:
                q, _ = ref.costs(t, gw, gh)
                assert path_costs(lib, h, gw, gh) == q, (kw, gw, gh)
                assert all(1 <= v <= 65536 for v in q)
                seen.add(q)
    assert (1, 1, 1) in seen and (65536, 65536, 65536) in seen
    assert any(qx == qy for qx, qy, _ in seen) and any(qx != qy for qx, qy, _ in seen)
    with Handle(lib) as h:
        q = (C.c_int32 * 3)()
        for args in ((None, 8, 8, q), (h, 8, 8, None), (h, 0, 8, q), (h, 8, 129, q)):
            assert lib.kb_path_costs(*args) == nat.KB_EINVAL and b'kb_path_costs' in lib.kb_last_error()


def test_kernel_uses_no_scratch_and_spills_nothing(lib):
    """The plane stays in LDS and the neighbours in registers: a zero private segment and zero spill counts in the metadata of
    the code object that was linked."""
    found = kernel_metadata('kb_paths_kernel')
    assert len(found) >= 1, found
    for name, fields in found:
        for key in ('.private_segment_fixed_size', '.sgpr_spill_count', '.vgpr_spill_count'):
            assert fields[key] == 0, (name, key, fields[key])


# ---- the restatement is the intended quantity ------------------------------------------------------------------------------
def bellman(aux, step):
    """D of every free reached cell that is no source is the least D(b) + w_k over the allowed moves, next the lowest k that
    attains it; sources are 0; a free cell without a path has no reached neighbour it may move to.  Returns the largest
    number of directions tied for next in one cell."""
    D, free, src, q = aux['D'], aux['free'], aux['src'], aux['q']
    w = ref.weights(q)
    gh, gw = free.shape
    most = 0
    for ay in range(gh):
        for ax in range(gw):
            if not free[ay, ax]:
                assert D[ay, ax] == ref.NONE and step[ay, ax] == -3
                continue
            vals = [(int(D[ay + ref.DIRS[k][1], ax + ref.DIRS[k][0]]) + w[k], k) for k in range(8)
                    if ref.allowed(free, ax, ay, k) and D[ay + ref.DIRS[k][1], ax + ref.DIRS[k][0]] != ref.NONE]
            if src[ay, ax]:
                assert D[ay, ax] == 0 and step[ay, ax] == -1
            elif D[ay, ax] == ref.NONE:
                assert not vals and step[ay, ax] == -2
            else:
                least = min(v for v, _ in vals)
                assert D[ay, ax] == least > 0
                tied = [k for v, k in vals if v == least]
                assert step[ay, ax] == tied[0]
                most = max(most, len(tied))
    return most


def zeros(n):
    return np.zeros(n, dtype=f32)


def test_mixed_scene_is_bellman_and_shows_every_flag(tab):
    gw, gh, source, blocked, xy, th = ref.mixed_scene()
    x, y = ((xy[:, k] * 25.0).astype(f32) for k in (0, 1))
    w, aux = ref.restate_env(tab, gw, gh, source, blocked, 0, 0.0, x, y, th.astype(f32))
    q = aux['q']
    assert q[0] != q[1] and q == ref.costs(tab, 7, 5)[0]        # the non-square grid
    assert bellman(aux, w.step) >= 2                            # a cell with two or more directions tied for next
    assert sorted(set(aux['flag'].tolist())) == [0, 1, 2, 3] and w.bots[:, 3].tolist() == [1, 0, 2, 3, 3, 0, 3]
    assert not aux['src'][2, 5] and source[2, 5]                # a blocked source is none
    assert np.isposinf(w.bots[[3, 4, 6], 0]).all() and (ref.bits(w.bots[[0, 3, 4, 6], 1:3]) == 0).all()
    assert w.bots[2, 0] > 0 and np.isposinf(w.dist[2, 4]) and w.step[2, 4] == -3
    assert (w.step[:, 6] == -2).all() and np.isposinf(w.dist[:, 4:]).all()
    # the stats are those of the rows
    fin = np.isfinite(w.bots[:, 0])
    assert w.stats[0] == fin.sum() == 4 and w.stats[3] == (aux['D'] != ref.NONE).sum() == 20 and w.stats[2] == w.bots[fin, 0].max()
    # a unit direction in the kilobot's frame
    n2 = w.bots[:, 1].astype(np.float64) ** 2 + w.bots[:, 2].astype(np.float64) ** 2
    assert np.allclose(n2[[1, 2, 5]], 1.0, atol=1e-6)


@pytest.mark.parametrize('gw,gh', [(33, 31), (7, 5), (1, 7), (5, 1), (1, 1)])
def test_serpentine_is_bellman_and_long(tab, gw, gh):
    blocked, source = ref.serpentine(gw, gh), ref.mask_of(gw, gh, [(0, 0)])
    w, aux = ref.restate_env(tab, gw, gh, source, blocked, 0, 0.0, zeros(1), zeros(1), zeros(1))
    bellman(aux, w.step)
    assert (aux['D'][aux['free']] != ref.NONE).all()            # one corridor: every free cell is reached
    if (gw, gh) == (33, 31):
        # the longest shortest path, in moves: follow next from the farthest cell
        ay, ax = np.unravel_index(np.argmax(aux['D']), aux['D'].shape)
        moves = 0
        while w.step[ay, ax] >= 0:
            dx, dy = ref.DIRS[w.step[ay, ax]]
            ax, ay, moves = ax + dx, ay + dy, moves + 1
        assert w.step[ay, ax] == -1 and moves >= 4 * max(gw, gh), moves


def test_corner_rule_changes_the_distances(tab):
    gw, gh = 7, 5
    blocked, source = ref.corner_scene(gw, gh), ref.mask_of(gw, gh, [(0, 0)])
    w, aux = ref.restate_env(tab, gw, gh, source, blocked, 0, 0.0, zeros(1), zeros(1), zeros(1))
    bellman(aux, w.step)
    assert blocked[1, 3] and blocked[2, 2] and not blocked[1, 2] and not blocked[2, 3]      # touching at a corner
    cut = ref.dijkstra(aux['free'], aux['src'], aux['q'], corner=False)
    assert (cut != aux['D']).any() and (cut <= aux['D'])[aux['free']].all() and (aux['D'][aux['free']] != ref.NONE).all()
    assert cut[2, 3] < aux['D'][2, 3]


def test_no_source_and_all_blocked(tab):
    x, y, th = zeros(3), zeros(3), zeros(3)
    for source, blocked in ((np.zeros((5, 7), np.uint8), None), (np.ones((5, 7), np.uint8), np.ones((5, 7), np.uint8))):
        w, aux = ref.restate_env(tab, 7, 5, source, blocked, 0, 0.0, x, y, th)
        assert np.isposinf(w.dist).all() and (w.step == (-2 if blocked is None else -3)).all()
        assert (w.bots[:, 3] == 3).all() and np.isposinf(w.bots[:, 0]).all() and (ref.bits(w.bots[:, 1:3]) == 0).all()
        assert (ref.bits(w.stats) == 0).all()


@pytest.mark.parametrize('name', ['disc', 'boxes', 'forms'])
def test_object_part_is_the_or_of_the_grid_planes(lib, name):
    """With clear_m == 0 the blocked plane of a set of objects is the OR of their kb_sense_grid planes; with a clearance it
    contains it, and the cells it adds are those whose centre is within the clearance of the outline."""
    kw, centres = objects_ref.object_sets()[name]
    _, _, objs, oth = objects_ref.spawn_over_objects(1, 1, centres, seed=5)
    ox, oy = ((objs[0, :, k] * 25.0).astype(f32) for k in (0, 1))
    ot = oth[0].astype(f32)
    with Handle(lib, **kw) as h:
        t = objects_ref.tables(nat.outline(h))
    M = t['M']
    for gw, gh in ((64, 48), (7, 5)):
        masks, dist_m = grid_ref.object_masks(t, gw, gh, ox, oy, ot)
        for objects in sorted({(1 << M) - 1, 1, (1 << M) - 2 if M > 1 else 0, 0}):
            chosen = [m for m in range(M) if objects >> m & 1]
            want = np.zeros((gh, gw), dtype=bool)
            for m in chosen:
                want |= masks[m] != 0
            got = ref.object_block(t, gw, gh, objects, 0.0, ox, oy, ot)
            assert np.array_equal(got, want), (name, gw, gh, objects)
            wide = ref.object_block(t, gw, gh, objects, 0.0165, ox, oy, ot)
            assert (wide | ~got).all()
            if chosen:
                near = np.min([dist_m[m] for m in chosen], 0)
                assert wide[near < 0.0164].all() and not (wide & ~got)[near > 0.0166].any()
        if (gw, gh) == (64, 48):
            assert want.any() and not want.all() and (wide & ~got).any()


def test_path_cells_is_the_cell_rule(tab):
    rng = np.random.RandomState(3)
    special = [[-1.0, -0.75], [1.0, 0.75], [1.0, -0.75], [0.0, 0.0], [-1.0, 0.3], [0.2, 0.75], [-1.2, 0.0], [3.0, 3.0], [-1e6, 1e6],
               [float('nan'), 0.1], [0.1, float('nan')], [2.0 / 7 - 1.0, 0.3 - 0.75]]
    pts = np.concatenate([np.array(special), rng.uniform(-1.1, 1.1, size=(40, 2)) * [1.0, 0.75]]).astype(f32)
    for gw, gh in ((7, 5), (64, 48), (1, 1), (128, 128), (1, 7)):
        mask = nat.path_cells(tab['arena'], pts, gw, gh)
        assert mask.dtype == np.uint8 and mask.shape == (1, gh, gw)
        ix, iy = grid_ref.cells(tab, gw, gh, pts[:, 0] * f32(25.0), pts[:, 1] * f32(25.0))
        want = np.zeros((gh, gw), dtype=np.uint8)
        want[iy, ix] = 1
        assert np.array_equal(mask[0], want), (gw, gh)
    per_env = nat.path_cells(tab['arena'], np.stack([pts[:3], pts[3:6]]), 7, 5)
    assert per_env.shape == (2, 5, 7) and np.array_equal(per_env[1], nat.path_cells(tab['arena'], pts[3:6], 7, 5)[0])
    for bad in (np.zeros((3,)), np.zeros((3, 3)), np.zeros((2, 2, 2, 2))):
        with pytest.raises(ValueError):
            nat.path_cells(tab['arena'], bad, 7, 5)
    with pytest.raises(ValueError):
        nat.path_cells(tab['arena'], pts, 0, 5)


def test_checks_of_the_python_arguments():
    assert nat.check_paths(64, 48) == (64, 48, 0.0) and nat.check_paths(1, 128, 0.0165) == (1, 128, 0.0165)
    for bad in ((0, 4), (4, 129), (True, 4), (4, 4, -0.1), (4, 4, float('nan')), (4, 4, float('inf'))):
        with pytest.raises(ValueError):
            nat.check_paths(*bad)
    assert nat.check_path_objects('all', 4) == 15 and nat.check_path_objects('all', 0) == 0 and nat.check_path_objects(5, 4) == 5
    assert nat.check_path_objects((0, 3), 4) == 9 and nat.check_path_objects((), 4) == 0 and nat.check_path_objects(0, 0) == 0
    for bad in (('some', 4), (16, 4), (-1, 4), ((4,), 4), (True, 4), (1, 0)):
        with pytest.raises(ValueError):
            nat.check_path_objects(*bad)


def test_batched_env_checks_path_obs():
    import torch
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    from tests.oracle_backend import OracleBackend
    env = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3)
    env.reset()
    a = torch.zeros(3, 16, 2)
    a[..., 0] = 0.01
    assert env.step(a)[3] == {} and env.path_obs is None
    for call in (env.paths, lambda: env.set_path_goal(cells=np.zeros((5, 7))), lambda: env.set_path_blocked(None)):
        with pytest.raises(ValueError):
            call()
    for bad in (5, (64,), (64, 48, 0.1, 1), (0, 48), (64, 129), ('a', 'b'), (True, 8), (64, 48, -1.0), (64, 48, float('nan'))):
        with pytest.raises(ValueError):
            BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, path_obs=bad)
    ok = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3, path_obs=(7, 5, 0.0165))
    assert ok.path_obs == (7, 5) and ok._observe_kw['path_obs']['clearance_m'] == 0.0165
    assert torch.equal(ok.reset(), BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3).reset())
    assert BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, path_obs=[32, 24]).path_obs == (32, 24)
    goal = ok._observe_kw['path_obs']['source']
    assert goal.dtype == torch.uint8 and tuple(goal.shape) == (3, 5, 7) and not goal.any()
    ok.set_path_goal(cells=ref.mask_of(7, 5, [(1, 2)]))
    goal = ok._observe_kw['path_obs']['source']
    assert tuple(goal.shape) == (3, 5, 7) and goal.sum() == 3 and goal[:, 2, 1].all()
    ok.set_path_blocked(np.ones((3, 5, 7), dtype=bool))
    assert ok._observe_kw['path_obs']['blocked'].dtype == torch.uint8 and ok._observe_kw['path_obs']['blocked'].all()
    ok.set_path_blocked(None)
    assert ok._observe_kw['path_obs']['blocked'] is None
    for bad in (dict(), dict(points_m=[[0.0, 0.0]], cells=np.zeros((5, 7))), dict(cells=np.zeros((7, 5))), dict(cells=np.zeros((2, 5, 7)))):
        with pytest.raises(ValueError):
            ok.set_path_goal(**bad)
