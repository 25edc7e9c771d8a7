"""kb_sense_coverage without a GPU: the symbol is exported, bound and declared, the host-side validation answers in the
header's order (arguments before the bound check, so none of it needs a device), the kernel has no private segment and no
spill (the code object's metadata), and the numpy restatement (tests/coverage_ref.py) is the intended quantity: the cells
of an env are shared out among its candidates, the owner is a nearest candidate in float64 up to the rounding of d2, and
the cost is the exact sum of the quantised terms.  The scenes of the GPU tests (tests/coverage_scenes.py) hold what they
are there for, checked here on the restatement alone.  BatchedKilobotsEnv checks coverage_obs at construction."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from tests import coverage_ref as ref
from tests import coverage_scenes as CS
from tests import grid_ref
from tests import objects_ref
from tests.host_common import abi_mismatches, Handle, lib, prototypes, tab  # noqa: F401
from tests.sensing_common import kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(1, 1), (3, 2), (7, 5), (64, 48), (127, 95), (128, 128)]
U = 2.0 ** -24      # the unit roundoff of float32


def test_symbol_is_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, 'include', 'kilobots_hip.h')).read()
    assert re.search(r'\bint\s+kb_sense_coverage\s*\(', hdr)
    assert 'kb_sense_coverage' in nat.EXPORTS and hasattr(lib, 'kb_sense_coverage')
    assert lib.kb_sense_coverage.argtypes is not None and len(lib.kb_sense_coverage.argtypes) == 9
    assert set(re.findall(r'\b(kb_[a-z_]+)\s*\(', hdr)) == set(nat.EXPORTS)
    ret, params = prototypes()['kb_sense_coverage']
    assert ret.strip() == 'int' and len(params) == 9
    assert abi_mismatches(nat.SIGNATURES, lambda name: (getattr(lib, name).restype, getattr(lib, name).argtypes)) == []


def test_check_coverage():
    assert nat.check_coverage(64, 48) == (64, 48) and nat.check_coverage(1, 128) == (1, 128) and nat.check_coverage(128.0, 1) == (128, 1)
    for bad in ((0, 4), (4, 0), (129, 4), (4, 129), (-1, 4), (True, 4), ('a', 4)):
        with pytest.raises(ValueError):
            nat.check_coverage(*bad)


def test_validation_on_an_unbound_handle(lib):
    """Nothing here launches: no pointer is dereferenced on the host.  The errors come in the header's order: NULL sim, gw /
    gh, all outputs NULL, a d_cell off 16 bytes; legal arguments reach the bound check."""
    out, odd, sel = C.c_void_p(0x1000), C.c_void_p(0x1004), C.c_void_p(0x3000)
    with Handle(lib) as h:
        bad = [
            ('NULL sim', (None, 8, 8, None, out, out, out, out), b'NULL handle'),
            ('NULL sim before a bad grid', (None, 0, 8, None, out, out, out, out), b'NULL handle'),
            ('NULL sim before no output', (None, 8, 8, None, None, None, None, None), b'NULL handle'),
            ('gw = 0', (h, 0, 8, None, out, out, out, out), b'KB_GRID_MAX_SIDE'),
            ('gh = 0', (h, 8, 0, None, out, out, out, out), b'KB_GRID_MAX_SIDE'),
            ('gw too large', (h, 129, 8, sel, out, None, None, None), b'KB_GRID_MAX_SIDE'),
            ('gh too large', (h, 8, 129, None, None, out, None, None), b'KB_GRID_MAX_SIDE'),
            ('negative gw', (h, -3, 8, None, out, out, out, out), b'KB_GRID_MAX_SIDE'),
            ('the grid before no output', (h, 8, 129, None, None, None, None, None), b'KB_GRID_MAX_SIDE'),
            ('the grid before the alignment', (h, 129, 8, None, None, None, odd, None), b'KB_GRID_MAX_SIDE'),
            ('no output', (h, 8, 8, None, None, None, None, None), b'all NULL'),
            ('no output, with a selection', (h, 128, 128, sel, None, None, None, None), b'all NULL'),
            ('d_cell off 16 bytes', (h, 8, 8, None, out, out, odd, out), b'16-byte'),
            ('d_cell alone off 16 bytes', (h, 1, 1, sel, None, None, C.c_void_p(0x1008), None), b'16-byte'),
        ]
        for what, args, word in bad:
            lib.kb_sense_neighbors(None, 0.07, 8, out, out, out, None)     # (leaves a message that the next call must replace)
            assert lib.kb_sense_coverage(*args, None) == nat.KB_EINVAL, what
            msg = lib.kb_last_error()
            assert msg and b'kb_sense_coverage' in msg and word in msg, (what, msg)
        # legal arguments reach the bound check: each output alone (the others float aligned at the most), all, with a selection
        for args in ((8, 8, None, out, out, out, out), (128, 128, sel, odd, odd, out, odd), (1, 1, None, odd, None, None, None),
                     (127, 95, None, None, odd, None, None), (64, 48, sel, None, None, out, None), (3, 2, None, None, None, None, odd)):
            assert lib.kb_sense_coverage(h, *args, None) == nat.KB_ENOTBOUND, args
            assert b'kb_sense_coverage' in lib.kb_last_error() and b'kb_bind' in lib.kb_last_error()


def test_kernel_uses_no_scratch_and_spills_nothing(lib):
    """The running best stays in registers and the accumulators in LDS: a zero private segment and zero spill counts in the
    metadata of the code object that was linked."""
    found = kernel_metadata('coverage')
    assert len(found) >= 1 and all('kb_coverage_kernel' in n for n, _ in found), found
    for name, fields in found:
        for key in ('.private_segment_fixed_size', '.sgpr_spill_count', '.vgpr_spill_count'):
            assert fields[key] == 0, (name, key, fields[key])


def squared_distances_f64(tab, gw, gh, x, y):
    """[gh * gw, N] float64: the squared distances of the float32 cell centres from the float32 poses, in double."""
    cx, cy = grid_ref.centres(tab, gw, gh)
    ex = x.astype(np.float64)[None] - cx.astype(np.float64)[:, None]
    ey = y.astype(np.float64)[None] - cy.astype(np.float64)[:, None]
    return ex * ex + ey * ey


def restated_is_intended(tab, gw, gh, x, y, th, sel):
    """The properties of the restatement on one scene and grid; returns it."""
    w = ref.restate(tab, gw, gh, x, y, th, sel)
    E, N = x.shape
    assert w.owner.dtype == np.int32 and w.owner.shape == (E, gh, gw) and w.dist.dtype == np.float32 and w.dist.shape == (E, gh, gw)
    assert w.cells.dtype == np.float32 and w.cells.shape == (E, N, 4) and w.stats.dtype == np.float32 and w.stats.shape == (E, 2)
    # The float32 d2 = fl(fl(ex * ex) + fl(ey * ey)) with ex = fl(x - cx), ey likewise: each offset carries one rounding, its
    # square two more and the sum a fourth, so d2 = D (1 + t) with |t| <= (1 + U)^4 - 1 =: G for the exact D (no underflow:
    # the offsets of distinct float32 numbers of this size are far above 2^-63).  If o beats b in float32, then
    # D_o (1 - G) <= d2_o <= d2_b <= D_b (1 + G), i.e. D_o - D_b <= G (D_o + D_b): two candidates may be taken for one another
    # only if their float64 distances differ by less than that.  (The float64 evaluation itself errs by 2^-51 relative: four
    # orders of magnitude below G, covered by evaluating G with 4.001 U.)
    G = 4.001 * U
    for e in range(E):
        cand = np.arange(N) if sel is None else np.flatnonzero(sel[e])
        own = w.owner[e].ravel()
        if len(cand) == 0:
            assert (own == -1).all() and np.isposinf(w.dist[e]).all() and not ref.bits(w.cells[e]).any() and np.isposinf(w.stats[e]).all()
            continue
        assert np.isin(own, cand).all()
        n = w.cells[e, :, 2]
        assert n.sum(dtype=np.float64) == gw * gh and np.array_equal(n, np.bincount(own, minlength=N).astype(np.float32))
        assert not ref.bits(w.cells[e][n == 0]).any()
        D = squared_distances_f64(tab, gw, gh, x[e], y[e])[:, cand]
        Do, Db = D[np.arange(gw * gh), np.searchsorted(cand, own)], D.min(1)
        assert (Do - Db <= G * (Do + Db)).all(), (gw, gh, e, float((Do - Db - G * (Do + Db)).max()))
        # the distance plane is the owner's: sqrt and the division round once each, so its square is D (1 + t), |t| < G + 4.1 U
        d2 = (w.dist[e].ravel().astype(np.float64) * 25.0) ** 2
        assert (np.abs(d2 - Do) <= (G + 4.1 * U) * Do).all()
        # the cost: the float64 sum of the quantised terms is exact below 2^53
        x32, y32 = x[e, own], y[e, own]
        cx, cy = grid_ref.centres(tab, gw, gh)
        ex, ey = x32 - cx, y32 - cy
        q = ref.quantised(ex * ex + ey * ey)
        acc = q.astype(np.float64).sum()
        assert acc < 2.0 ** 53 and acc == int(q.sum(dtype=np.int64))
        assert w.stats[e, 0] == (np.float32(acc) / np.float32(65536.0)) / np.float32(625.0)
        assert w.stats[e, 1] == w.dist[e].max() and w.stats[e, 1] == w.cells[e, :, 3].max()
    return w


@pytest.mark.parametrize('gw,gh', GRIDS)
def test_restatement_on_the_wall_scene(tab, gw, gh):
    """Kilobots outside the arena take part with their true positions, and some of them own cells."""
    x, y, th, sel = CS.walls()
    w = restated_is_intended(tab, gw, gh, x, y, th, sel)
    ar = tab['arena']
    outside = (x < ar[0]) | (x > ar[1]) | (y < ar[2]) | (y > ar[3])
    assert outside.any(1).all()
    # (from 64 x 48 on: the kilobots outside lie at most 0.75 world units beyond a wall, which is nearer to the edge centres
    # than the kilobots inside only where a cell is at most about that wide; on the coarse grids they may own nothing)
    if gw >= 64:
        assert all((w.cells[e, outside[e], 2] > 0).any() for e in range(x.shape[0]))


def test_restatement_on_the_tie_scene(tab):
    """On 50 x 75 the constants are exact and whole columns, rows and diagonals of cell centres are equidistant from two
    kilobots, the centre (-0.5, -0.5) from four: the lower index owns them, whichever kilobot that is in the env."""
    x, y, th, sel = CS.ties()
    gw, gh = CS.TIE_GRID
    xmin, ymin, cw, ch, _, _ = grid_ref.constants(tab, gw, gh)
    assert (float(xmin), float(ymin), float(cw), float(ch)) == (-25.0, -18.75, 1.0, 0.5)
    w = restated_is_intended(tab, gw, gh, x, y, th, sel)
    for e in range(3):
        k = ref.keys(tab, gw, gh, x[e], y[e], np.arange(7))
        least = (k >> np.uint64(32)).min(1)
        tied = ((k >> np.uint64(32)) == least[:, None]).sum(1)
        assert (tied >= 2).sum() >= 50 and tied.max() >= 4, (e, int((tied >= 2).sum()), int(tied.max()))
        first = ((k >> np.uint64(32)) == least[:, None]).argmax(1)
        assert np.array_equal(w.owner[e].ravel(), first)
    centre = (36, 24)       # cy = -18.5 + 0.5 * 36, cx = -24.5 + 24
    assert w.owner[0][centre] == 0 and w.owner[1][centre] == 3 and w.dist[0][centre] == np.float32(2.0) / np.float32(25.0)
    assert 1 in np.unique(w.owner[2]) and 3 not in np.unique(w.owner[2])      # of the two that share a point the lower owns everything


def test_restatement_on_the_lone_kilobot(tab):
    x, y, th, sel = CS.one()
    for gw, gh in ((64, 48), (1, 1)):
        w = restated_is_intended(tab, gw, gh, x, y, th, sel)
        assert not w.owner.any() and (w.cells[:, 0, 2] == gw * gh).all()


@pytest.mark.parametrize('gw,gh', CS.DENSE_GRIDS)
def test_restatement_on_the_dense_scene(tab, gw, gh):
    """The lattice has a pitch of 1.125 world units: on 64 x 48 (cells of 0.78) and 128 x 128 every kilobot owns a cell, on
    16 x 12 (cells of 3.125) most own nothing."""
    x, y, th, sel = CS.dense()
    w = restated_is_intended(tab, gw, gh, x, y, th, sel)
    idle = (w.cells[..., 2] == 0).sum(1)
    assert (idle > 512).all() if (gw, gh) == (16, 12) else not idle.any()


def test_restatement_on_the_select_scene(tab):
    x, y, th, sel = CS.select()
    assert sel.dtype == np.uint8 and (sel != 0).sum(1).tolist()[1:] == [1, 0] and 100 < (sel[0] != 0).sum() < 233 and sel.max() > 1
    w = restated_is_intended(tab, 64, 48, x, y, th, sel)
    assert (w.owner[1] == 217).all() and (w.owner[2] == -1).all()
    assert not ref.bits(w.cells[0][sel[0] == 0]).any()
    everyone = ref.restate(tab, 64, 48, x, y, th)
    assert (everyone.owner[0] != w.owner[0]).any() and (everyone.dist <= w.dist).all()


def test_batched_env_coverage_obs_without_a_gpu():
    import torch
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    from tests.oracle_backend import OracleBackend
    env = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3)
    env.reset()
    a = torch.zeros(3, 16, 2)
    a[..., 0] = 0.01
    assert env.step(a)[3] == {} and env.coverage_obs is None
    with pytest.raises(ValueError):
        env.coverage()
    for bad in (5, (64,), (64, 48, 1), (0, 48), (64, 129), ('a', 'b'), (True, 8)):
        with pytest.raises(ValueError):
            BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, coverage_obs=bad)
    ok = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3, coverage_obs=(64, 48))
    assert ok.coverage_obs == (64, 48)
    assert torch.equal(ok.reset(), BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3).reset())
    assert BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, coverage_obs=[32, 24]).coverage_obs == (32, 24)


# ---- what the search of kb_coverage_kernel does on a scene: its ring budget and cell indices, restated to hold the scenes to
# ---- the path they are there for (the results never come from here: tests/coverage_ref.py knows no ring)
def ring_budget(N, cells_w, cells_h):
    """The rings kb_coverage_kernel walks at the most before it scans all kilobots: k while (2 k + 1)^2 * COST <= N."""
    src = open(os.path.join(ROOT, 'gym_kilobots_amd', 'csrc', 'kb_sense.h')).read()
    cost = int(re.search(r'#define\s+KB_COVERAGE_RING_COST\s+(\d+)', src).group(1))
    rings = 0
    while rings < cells_w + cells_h and (2 * rings + 1) ** 2 * cost <= N:
        rings += 1
    return rings


def broadphase_cells(tab, cell, cells_w, cells_h, x, y):
    """(cx, cy) int: the clamped broadphase cell of float32 coordinates, by the fp32 expressions of kb_build_cell_lists."""
    f = np.float32
    inv = f(1.0) / f(cell)
    bx = np.floor((f(x) - tab['arena'][0]) * inv).astype(np.int64)
    by = np.floor((f(y) - tab['arena'][2]) * inv).astype(np.int64)
    return np.clip(bx, 0, cells_w - 1), np.clip(by, 0, cells_h - 1)


def reach(d, cell):
    """sense_reach (kb_sense.h) of a distance."""
    f = np.float32
    return int(np.floor(f(d) * (f(1.0) / f(cell)) + f(1e-3))) + 1


def test_one_kilobot_and_small_ties_never_settle_in_a_ring():
    """The budget gives one kilobot no ring and seven kilobots one, and ring 0 alone settles nothing (the reach is at least 1):
    ties() and one() test the scan of all kilobots, not a search across the grid.  ring_ties() and far_corner() test the rings."""
    assert ring_budget(1, 58, 43) == 0 and ring_budget(7, 58, 43) == 1 and reach(0.0, 0.875) == 1
    assert ring_budget(CS.RING_TIE_BOTS, 58, 43) == 4 and ring_budget(1024, 15, 11) == 11 and ring_budget(1024, 58, 43) == 11


def test_restatement_on_the_ring_tie_scene(tab):
    """Tied cells exist that the rings settle, with the tied kilobots in different rings: in env 0 the lower index lies in the
    OUTER ring for outer rings 1, 2 and 3 -- a search that stopped a ring early, or took a tie by the order it met the kilobots
    in, names another owner --, in env 1 in the inner one."""
    x, y, th, sel = CS.ring_ties()
    gw, gh = CS.TIE_GRID
    N = CS.RING_TIE_BOTS
    rings = ring_budget(N, 58, 43)
    assert rings >= 2
    w = restated_is_intended(tab, gw, gh, x, y, th, sel)
    cx, cy = grid_ref.centres(tab, gw, gh)
    cbx, cby = broadphase_cells(tab, 0.875, 58, 43, cx, cy)
    seen = {0: set(), 1: set(), 2: set()}
    for e in range(3):
        k = ref.keys(tab, gw, gh, x[e], y[e], np.arange(N))
        d2bits = k >> np.uint64(32)
        least = d2bits.min(1)
        bx, by = broadphase_cells(tab, 0.875, 58, 43, x[e], y[e])
        for c in np.flatnonzero((d2bits == least[:, None]).sum(1) >= 2):
            tied = np.flatnonzero(d2bits[c] == least[c])
            ring = np.maximum(np.abs(bx[tied] - cbx[c]), np.abs(by[tied] - cby[c]))
            d = np.sqrt(least[c].astype(np.uint32).view(np.float32))
            if ring.max() == ring.min() or max(reach(d, 0.875), ring.max()) > rings - 1:
                continue        # (one ring, or the scan settles it)
            assert w.owner[e].ravel()[c] == tied[0]
            seen[e].add((int(ring[0]), int(ring.max())))        # (the owner's ring, the outermost ring of the tie)
    print('rings of (owner, outermost tied kilobot) per env:', seen)
    assert {(1, 1), (2, 2), (3, 3)} <= seen[0], seen[0]                  # the owner is met last, one to three rings out
    assert {(0, 1), (1, 2), (2, 3)} <= seen[1], seen[1]                  # the owner is met first
    assert len(seen[2]) >= 2


def test_restatement_on_the_far_corner_scene(lib):
    """With all kilobots in one corner cell of 15 x 11 cells, centres find them in the very ring that holds the far corner of
    the grid from their own cell, inside the budget of eleven rings: the search ends on that ring; others lie further and scan."""
    from tests import geometry_scenes as GS
    with Handle(lib, **CS.FAR_CORNER_KW) as h:
        tab = objects_ref.tables(nat.outline(h))
    cell, cw_, ch_ = GS.grid(2.0, 1.5, CS.FAR_CORNER_KW['bot_radius'])
    assert (cell, cw_, ch_) == (3.5, 15, 11)
    x, y, th, sel = CS.far_corner()
    rings = ring_budget(1024, cw_, ch_)
    for gw, gh in ((64, 48), (7, 5)):
        restated_is_intended(tab, gw, gh, x, y, th, sel)
        cbx, cby = broadphase_cells(tab, cell, cw_, ch_, *grid_ref.centres(tab, gw, gh))
        kfull = np.maximum(np.maximum(cbx, cw_ - 1 - cbx), np.maximum(cby, ch_ - 1 - cby))
        for e, corner in enumerate(((0, 0), (cw_ - 1, ch_ - 1))):
            bx, by = broadphase_cells(tab, cell, cw_, ch_, x[e], y[e])
            assert (bx == corner[0]).all() and (by == corner[1]).all()
            ring = np.maximum(np.abs(cbx - corner[0]), np.abs(cby - corner[1]))
            ends_there, scans = (ring == kfull) & (kfull <= rings - 1), ring > rings - 1
            print('%d x %d env %d: %d centres end on the ring of the far corner, %d scan' % (gw, gh, e, ends_there.sum(), scans.sum()))
            assert ends_there.sum() >= gw * gh // 8 and scans.sum() >= 1
