"""kb_sense_edges without a GPU: the symbol is exported, declared and bound, the host-side validation answers in the header's
order (arguments before the bound check, so none of it needs a device), the kernel keeps no scratch and spills nothing (the
code object's metadata), the numpy restatement (tests/edges_ref.py) has the properties of the definition -- a symmetric edge
set, the same distance bits in both directions, the counts of the neighbours restatement, strictly ascending rows -- its
memory-contract function does what the header says on hand-made offsets, and the scenes of tests/test_edges_gpu.py are shown
not to be vacuous, on the restatement alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from tests import edges_ref as ref
from tests.host_common import Handle, lib  # noqa: F401
from tests.sensing_common import SWEEP, kernel_metadata, sweep_scene, wall_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPLETE_N = (32, 33, 65, 257, 1024)        # the complete-graph shapes of the GPU tests, all at (2, N, 4.0)
WALL_R = (0.04, 0.09, 0.15)


def header_block():
    hdr = open(os.path.join(ROOT, 'include', 'kilobots_hip.h')).read()
    return hdr, hdr[hdr.index('The whole IR-range graph on the CURRENT poses'):hdr.index('int kb_sense_edges')]


def test_symbol_is_exported_declared_and_bound(lib):
    hdr, block = header_block()
    assert re.search(r'\bint\s+kb_sense_edges\s*\(', hdr)
    decl = hdr[hdr.index('int kb_sense_edges'):]
    decl = decl[:decl.index(';')]
    assert len(decl[decl.index('(') + 1:decl.rindex(')')].split(',')) == 9
    assert 'kb_sense_edges' in nat.EXPORTS and hasattr(lib, 'kb_sense_edges')
    assert lib.kb_sense_edges.argtypes is not None and len(lib.kb_sense_edges.argtypes) == 9
    assert lib.kb_sense_edges.argtypes[3] is C.c_int64 and lib.kb_sense_edges.restype is C.c_int
    assert set(re.findall(r'\b(kb_[a-z_]+)\s*\(', hdr)) == set(nat.EXPORTS)
    assert 'no reference counterpart' in block.lower()
    assert 'as kb_sense_neighbors' in block and 'ASCENDING j' in block
    # the header says which way capacity == 0 without d_count goes on an unbound handle: the bound check comes first
    assert 'on an unbound handle it answers KB_ENOTBOUND' in ' '.join(block.replace('*', ' ').split())


def test_validation_on_an_unbound_handle(lib):
    """Nothing here launches: the pointers are never dereferenced on the host (any non-NULL value will do).  Every bad call
    has exactly one thing wrong behind the things that are checked before it, and names what it is."""
    off, src, dst, rel, cnt = (C.c_void_p(0x1000 * k) for k in range(1, 6))
    odd = C.c_void_p(0x3004)        # (a d_rel off its 16 bytes: checked behind the bound check, as kb_sense_neighbors does)
    with Handle(lib) as h:
        bad = [
            ('NULL sim', (None, 0.1, off, 8, src, dst, rel, cnt, None), b'NULL argument'),
            ('NULL d_offsets', (h, 0.1, None, 8, src, dst, rel, cnt, None), b'NULL argument'),
            ('NULL d_offsets before the radius', (h, 0.0, None, 8, src, dst, rel, cnt, None), b'NULL argument'),
            ('radius = 0', (h, 0.0, off, 8, src, dst, rel, cnt, None), b'radius'),
            ('radius = -1', (h, -1.0, off, 8, src, dst, rel, cnt, None), b'radius'),
            ('radius = NaN', (h, float('nan'), off, 8, src, dst, rel, cnt, None), b'radius'),
            ('radius before the capacity', (h, 0.0, off, -1, src, dst, rel, cnt, None), b'radius'),
            ('capacity = -1', (h, 0.1, off, -1, src, dst, rel, cnt, None), b'capacity'),
            ('capacity = -2^40', (h, 0.1, off, -(1 << 40), src, dst, rel, cnt, None), b'capacity'),
            ('capacity before d_dst', (h, 0.1, off, -1, src, None, rel, cnt, None), b'capacity must not'),
            ('NULL d_dst with a capacity', (h, 0.1, off, 8, src, None, rel, cnt, None), b'NULL d_dst'),
            ('NULL d_dst before the alignment', (h, 0.1, off, 1 << 40, src, None, odd, cnt, None), b'NULL d_dst'),
        ]
        for what, args, word in bad:
            lib.kb_sense_neighbors(None, 0.07, 8, dst, rel, cnt, None)      # (leaves a message that the next call must replace)
            assert lib.kb_sense_edges(*args) == nat.KB_EINVAL, what
            msg = lib.kb_last_error()
            assert msg and b'kb_sense_edges' in msg and word in msg, (what, msg)
        # legal arguments reach the bound check -- optional outputs or not, a radius beyond the arena, a capacity beyond int32,
        # the counting call, and capacity == 0 without d_count, which would launch nothing: the header puts the bound check first.
        # A misaligned d_rel is reported behind the bound check and does not show here.
        legal = [(0.1, 8, src, dst, rel, cnt), (100.0, 8, None, dst, None, None), (1e-3, 1 << 40, src, dst, rel, None), (0.1, 0, None, None, None, cnt),
                 (0.1, 0, None, None, None, None), (0.1, 0, src, dst, rel, None), (0.1, 8, src, dst, odd, cnt)]
        for r, cap, ps, pd, pr, pc in legal:
            assert lib.kb_sense_edges(h, r, off, cap, ps, pd, pr, pc, None) == nat.KB_ENOTBOUND, (r, cap)
            assert b'kb_sense_edges' in lib.kb_last_error() and b'kb_bind' in lib.kb_last_error()


def test_check_edges_and_its_limits():
    assert nat.check_edges(0.1) == (0.1, None) and nat.check_edges(1, 0) == (1.0, 0)
    assert nat.check_edges(0.07, 1 << 33) == (0.07, 1 << 33)
    assert isinstance(nat.check_edges(0.1, 8.0)[1], int) and isinstance(nat.check_edges(0.1, np.int64(8))[1], int)
    for bad in ((0.0,), (-0.1,), (float('nan'),), (0.1, -1), (0.1, 2.5), (0.1, True)):
        with pytest.raises(ValueError):
            nat.check_edges(*bad)


def test_batched_env_edge_obs_without_a_gpu():
    import torch
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    from tests.oracle_backend import OracleBackend
    env = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3)
    env.reset()
    a = torch.zeros(3, 16, 2)
    a[..., 0] = 0.01
    assert env.step(a)[3] == {}
    assert env.edge_obs is None
    with pytest.raises(ValueError):
        env.edges()
    for bad in (0.0, -1.0, (0.1, -1), (0.1, 2.5), (0.1, 8, 1), (), 'far', (0.1, 'many')):
        with pytest.raises(ValueError):
            BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3, edge_obs=bad)
    assert BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3, edge_obs=0.1).edge_obs == (0.1, None)
    assert BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3, edge_obs=(0.1, 500)).edge_obs == (0.1, 500)


def test_no_scratch_and_no_spills():
    found = kernel_metadata('edges')
    assert len(found) == 1 and 'kb_edges_kernel' in found[0][0], found
    for name, fields in found:
        print(name, fields)
        assert fields == {'.private_segment_fixed_size': 0, '.sgpr_spill_count': 0, '.vgpr_spill_count': 0}, name


# ---- the restatement has the properties of the definition ------------------------------------------------------------------
def scene_list():
    return [('sweep', E, N, R) for E, N, R in SWEEP] + [('walls', 4, 96, R) for R in WALL_R]


def poses(kind, E, N):
    return ref.world(*(sweep_scene(E, N) if kind == 'sweep' else wall_scene(random_headings=True)))


@pytest.fixture(scope='module')
def restated():
    """(kind, E, N, R) -> ((x, y, th), restate(...)): computed once, shared and left unchanged."""
    out = {}
    for kind, E, N, R in scene_list():
        xyt = poses(kind, E, N)
        out[kind, E, N, R] = xyt, ref.restate(*xyt, R)
    return out


@pytest.mark.parametrize('kind,E,N,R', scene_list())
def test_restatement_properties(restated, kind, E, N, R):
    (x, y, th), (src, dst, rel, count, offsets) = restated[kind, E, N, R]
    nnz = len(src)
    assert src.dtype == dst.dtype == np.int32 and rel.dtype == np.float32 and rel.shape == (nnz, 4) and offsets.dtype == np.int64
    assert offsets[0] == 0 and offsets[-1] == nnz and np.array_equal(np.diff(offsets), count.ravel())
    assert np.array_equal(src, np.repeat(np.arange(E * N), count.ravel()))          # the rows are where the row pointer says
    assert (src // N == dst // N).all() and (src != dst).all()                      # edges stay inside an env, no loops
    # strictly ascending rows: inside a row dst grows, so (src, dst) as one key grows over the whole list
    key = src.astype(np.int64) * (E * N) + dst
    assert (np.diff(key) > 0).all()
    # the edge set is symmetric, and the distance has the same bits in both directions
    back = np.searchsorted(key, dst.astype(np.int64) * (E * N) + src)
    assert (back < nnz).all() and np.array_equal(src[back], dst) and np.array_equal(dst[back], src)
    assert np.array_equal(ref.bits(rel[:, 2]), ref.bits(rel[back, 2]))
    assert np.array_equal(ref.bits(rel[:, 3]), ref.bits(-rel[back, 3]))             # (a - b = -(b - a) exactly)
    # the counts, and the rows of at most 16, are those of the neighbours restatement
    from tests.sensing_checks import restate_neighbors
    index, nrel, ncount, _ = restate_neighbors(x, y, th, R, 16)
    assert np.array_equal(count, ncount)
    for r in np.flatnonzero(count.ravel() <= 16)[:200]:
        e, i = divmod(int(r), N)
        m, lo = int(count[e, i]), int(offsets[r])
        order = np.argsort(index[e, i, :m])
        assert np.array_equal(index[e, i, :m][order] + e * N, dst[lo:lo + m])
        assert np.array_equal(ref.bits(nrel[e, i, :m][order]), ref.bits(rel[lo:lo + m]))


def test_contract_on_hand_made_offsets():
    """Four rows with 1, 2, 1 and 0 edges against offsets that are negative and oversized, that give rows more than they have,
    that leave holes, that meet a capacity below nnz, and that descend."""
    x = np.array([[0.0, 1.0, 2.0, 50.0]], np.float32)
    y = np.zeros((1, 4), np.float32)
    th = np.array([[0.1, 0.2, 0.3, 0.4]], np.float32)
    true = ref.restate(x, y, th, 0.05)            # Rw = 1.25: 0-1, 1-2
    assert true[3].tolist() == [[1, 2, 1, 0]] and true[1].tolist() == [1, 0, 2, 1]
    before = (np.full(7, 9, np.int32), np.full(7, 9, np.int32), np.full((7, 4), 9, np.float32))
    src, dst, rel, owned = ref.contract(true, np.array([-3, 1, 3, 5, 1 << 40], np.int64), 7, before)
    # clipped to 0, 1, 3, 5, 7 -- row 0: [0, 1) its one; row 1: [1, 3) its two; row 2: [3, 5) its one, then the fill; row 3: [5, 7) has none: the fill
    assert dst.tolist() == [1, 0, 2, 1, -1, -1, -1] and src.tolist() == [0, 1, 1, 2, -1, -1, -1] and owned.all()
    assert (rel[4:] == 0).all() and not np.signbit(rel[4:]).any() and np.array_equal(ref.bits(rel[:4]), ref.bits(true[2]))
    src, dst, rel, owned = ref.contract(true, np.array([2, 3, 3, 3, 4], np.int64), 7, before)
    assert dst.tolist() == [9, 9, 1, -1, 9, 9, 9] and owned.tolist() == [False, False, True, True, False, False, False]
    src, dst, rel, owned = ref.contract(true, true[4], 3, tuple(b[:3] for b in before))       # the true offsets, a capacity below nnz
    assert dst.tolist() == [1, 0, 2] and owned.all()
    src, dst, rel, owned = ref.contract(true, np.array([9, 4, 2, 1, 0], np.int64), 7, before)      # descending: every row is empty
    assert dst.tolist() == [9] * 7 and not owned.any()


# ---- the scenes of tests/test_edges_gpu.py are not vacuous -----------------------------------------------------------------
def test_scenes_are_not_vacuous(restated):
    """Over the sweep and the wall scene: rows longer than the 16 slots of kb_sense_neighbors, empty rows, a batch without a
    single edge, complete rows; the table of the issue (kilobots with more than 16 neighbours, the longest row)."""
    counts = {k: v[1][3] for k, v in restated.items()}
    for k, c in sorted(counts.items()):
        print(k, 'nnz %d, longest row %d, %d rows above 16, %d empty, %d complete' % (c.sum(), c.max(), (c > 16).sum(), (c == 0).sum(), (c == k[2] - 1).sum()))
    c = counts['sweep', 8, 64, 0.3]
    assert ((c > 16).sum(), c.max()) == (417, 48)
    c = counts['sweep', 4, 1024, 0.1]
    assert ((c > 16).sum(), c.max()) == (473, 19)
    c = counts['walls', 4, 96, 0.15]
    assert ((c > 16).sum(), c.max()) == (104, 27)
    assert any((c == 0).any() and (c > 0).any() for c in counts.values())
    assert counts['sweep', 5, 1, 0.1].sum() == 0                                    # nnz == 0
    for k in (('sweep', 2, 7, 4.0), ('sweep', 2, 7, 0.5)):
        assert (counts[k] == k[2] - 1).any()                                        # complete rows at small N
    assert (counts['sweep', 2, 7, 4.0] == 6).all()
    x, y, th = poses('walls', 4, 96)
    assert (np.abs(x) > 25.0).any() and (np.abs(y) > 18.75).any()                   # some kilobots are outside: their cell indices clamp


@pytest.mark.parametrize('N', COMPLETE_N)
def test_complete_graph_shapes_are_complete(N):
    """(2, N, 4.0): 100 world units reach across the arena (50 x 37.5), so every row has N - 1 entries.  Counts only."""
    x, y, _ = ref.world(*sweep_scene(2, N))
    for e in range(2):
        assert (ref.in_range(x[e], y[e], 4.0)[0].sum(1) == N - 1).all()
