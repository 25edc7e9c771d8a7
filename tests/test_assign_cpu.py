"""kb_sense_assign without a GPU: the symbol is exported, bound and declared, the host-side validation answers in the header's
order (arguments before the bound check, so none of it needs a device), the kernel has no private segment and no spill (the
code object's metadata), and the numpy restatement (tests/assign_ref.py) is the intended quantity: the sorted walk and the
round process, which share nothing but d2, give the same matching on every scene, and the result is one-to-one, consistent
between its two sides and as large as the smaller side allows.  The scenes of the GPU tests (tests/assign_scenes.py) hold what
they are there for, checked here on the restatement alone.  BatchedKilobotsEnv checks target_match at construction."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from tests import assign_ref as ref
from tests import assign_scenes as AS
from tests import targets_ref
from tests.host_common import abi_mismatches, Handle, lib, prototypes  # noqa: F401
from tests.sensing_common import kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(a, b):
    return all(np.array_equal(ref.bits(p), ref.bits(q)) if p.dtype == np.float32 else np.array_equal(p, q) for p, q in zip(a, b))


@pytest.fixture(scope='module')
def restated():
    """{name: (scene, restatement)} of every scene, computed once."""
    return {name: (sc, ref.restate(*sc)) for name, sc in ((n, fn()) for n, fn in AS.SCENES.items())}


def test_symbol_is_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, 'include', 'kilobots_hip.h')).read()
    assert re.search(r'\bint\s+kb_sense_assign\s*\(', hdr)
    assert 'kb_sense_assign' in nat.EXPORTS and 'kb_sense_assign' in nat.OPTIONAL and hasattr(lib, 'kb_sense_assign')
    assert lib.kb_sense_assign.argtypes is not None and len(lib.kb_sense_assign.argtypes) == 14
    assert lib.kb_sense_assign.argtypes[4] is C.c_float and lib.kb_sense_assign.argtypes[5] is C.c_float
    assert set(re.findall(r'\b(kb_[a-z_]+)\s*\(', hdr)) == set(nat.EXPORTS)
    ret, params = prototypes()['kb_sense_assign']
    assert ret.strip() == 'int' and len(params) == 14
    assert abi_mismatches(nat.SIGNATURES, lambda name: (getattr(lib, name).restype, getattr(lib, name).argtypes)) == []


def test_check_assign():
    inf = float('inf')
    assert nat.check_assign(1, 0, None) == (1, 0.0, inf) and nat.check_assign(1024, 0.02, 0) == (1024, 0.02, 0.0)
    assert nat.check_assign(64.0, 1, inf) == (64, 1.0, inf) and nat.check_assign(8, 0.02, 0.25) == (8, 0.02, 0.25)
    for bad in ((0, 0.02, None), (1025, 0.02, None), (8, -0.01, None), (8, inf, None), (8, float('nan'), 0.1), (True, 0.02, None), (8, True, None),
                (8, 0.02, -0.1), (8, 0.02, float('nan')), (8, 0.02, -inf), (8, 0.02, True), (8, 0.02, 'c')):
        with pytest.raises(ValueError):
            nat.check_assign(*bad)


def test_validation_on_an_unbound_handle(lib):
    """Nothing here launches: no pointer is dereferenced on the host.  The errors come in the header's order: NULL sim or
    points, n_targets, tol_m, cutoff_m, all outputs NULL, a d_rel off 16 bytes; legal arguments reach the bound check."""
    pts, out, odd, sel = C.c_void_p(0x2000), C.c_void_p(0x1000), C.c_void_p(0x1004), C.c_void_p(0x3000)
    inf, nan = float('inf'), float('nan')
    none = (None,) * 5
    with Handle(lib) as h:
        bad = [
            ('NULL sim', (None, pts, 8, 0, 0.02, inf, None, None, out, out, out, out, out), b'NULL argument'),
            ('NULL points', (h, None, 8, 0, 0.02, inf, None, None, out, out, out, out, out), b'NULL argument'),
            ('NULL sim before bad n_targets', (None, pts, 0, 0, 0.02, inf, None, None, out, out, out, out, out), b'NULL argument'),
            ('NULL points before bad cutoff_m', (h, None, 8, 1, 0.02, -1.0, None, None, out, out, out, out, out), b'NULL argument'),
            ('n_targets = 0', (h, pts, 0, 0, 0.02, inf, None, None, out, out, out, out, out), b'KB_MAX_TARGETS'),
            ('n_targets too large', (h, pts, 1025, 1, 0.02, 0.1, sel, sel, out, None, None, None, None), b'KB_MAX_TARGETS'),
            ('n_targets before tol_m', (h, pts, 0, 0, -1.0, inf, None, None, out, out, out, out, out), b'KB_MAX_TARGETS'),
            ('n_targets before cutoff_m', (h, pts, -4, 0, 0.02, nan, None, None, out, out, out, out, out), b'KB_MAX_TARGETS'),
            ('negative tol_m', (h, pts, 8, 0, -0.01, inf, None, None, out, out, out, out, out), b'tol_m'),
            ('infinite tol_m', (h, pts, 8, 0, inf, inf, None, None, out, out, out, out, out), b'tol_m'),
            ('tol_m before cutoff_m', (h, pts, 8, 1, nan, -1.0, sel, None, out, out, out, out, out), b'tol_m'),
            ('tol_m before no output', (h, pts, 8, 0, nan, inf, None, None) + none, b'tol_m'),
            ('negative cutoff_m', (h, pts, 8, 0, 0.02, -0.01, None, None, out, out, out, out, out), b'cutoff_m'),
            ('cutoff_m of -inf', (h, pts, 8, 0, 0.02, -inf, None, None, out, out, out, out, out), b'cutoff_m'),
            ('cutoff_m that is no number', (h, pts, 8, 0, 0.02, nan, None, None, out, out, out, out, out), b'cutoff_m'),
            ('cutoff_m before no output', (h, pts, 8, 0, 0.02, nan, None, None) + none, b'cutoff_m'),
            ('cutoff_m before the alignment', (h, pts, 8, 0, 0.02, -1.0, None, None, None, odd, None, None, None), b'cutoff_m'),
            ('no output', (h, pts, 8, 0, 0.02, inf, None, None) + none, b'all NULL'),
            ('no output, with selections', (h, pts, 1024, 1, 0.0, 0.0, sel, sel) + none, b'all NULL'),
            ('no output before the alignment is looked at', (h, pts, 8, 0, 0.02, 0.5, None, None) + none, b'all NULL'),
            ('d_rel off 16 bytes', (h, pts, 8, 0, 0.02, inf, None, None, out, odd, out, out, out), b'16-byte'),
            ('d_rel alone off 16 bytes', (h, pts, 1, 1, 0.0, 0.0, sel, sel, None, C.c_void_p(0x1008), None, None, None), b'16-byte'),
        ]
        for what, args, word in bad:
            lib.kb_sense_neighbors(None, 0.07, 8, out, out, out, None)     # (leaves a message that the next call must replace)
            assert lib.kb_sense_assign(*args, None) == nat.KB_EINVAL, what
            msg = lib.kb_last_error()
            assert msg and b'kb_sense_assign' in msg and word in msg, (what, msg)
        # legal arguments reach the bound check: all outputs, each alone, the limits, no cutoff and a cutoff of zero
        for args in ((pts, 8, 0, 0.02, inf, None, None, out, out, out, out, out), (pts, 1024, 1, 0.0, 0.0, sel, sel, odd, out, odd, odd, odd),
                     (pts, 1, 0, 0.02, 0.1, None, None, odd, None, None, None, None), (pts, 5, 1, 1e30, 1e30, None, sel, None, out, None, None, None),
                     (pts, 5, 0, 0.02, inf, sel, None, None, None, odd, None, None), (pts, 5, 0, 0.02, 3.0, None, None, None, None, None, odd, None),
                     (odd, 5, 0, 0.02, inf, None, None, None, None, None, None, odd)):
            assert lib.kb_sense_assign(h, *args, None) == nat.KB_ENOTBOUND, args
            assert b'kb_sense_assign' in lib.kb_last_error() and b'kb_bind' in lib.kb_last_error()


def test_kernel_uses_no_scratch_and_spills_nothing(lib):
    """The running bests of a scan stay in registers and everything else in LDS: a zero private segment and zero spill counts
    in the metadata of the code object that was linked."""
    found = kernel_metadata('kb_assign_kernel')
    assert len(found) == 1, found
    for name, fields in found:
        for key in ('.private_segment_fixed_size', '.sgpr_spill_count', '.vgpr_spill_count'):
            assert fields[key] == 0, (name, key, fields[key])


def test_the_walk_equals_the_round_process(restated):
    """Two ways to M that share only d2: the sorted walk over all admissible pairs and the rounds of mutual choices."""
    assert set(restated) == set(AS.SCENES) and len(AS.SCENES) == len(AS.SMALL) + 1
    for name, (sc, w) in restated.items():
        assert sc.x.dtype == sc.y.dtype == sc.th.dtype == sc.points.dtype == np.float32, name
        assert same(w, ref.restate(*sc, matching='rounds')), name


def test_every_matching_is_one_to_one(restated):
    for name, (sc, w) in restated.items():
        E, N = sc.x.shape
        K = sc.points.shape[-2]
        assert w.index.shape == (E, N) and w.rel.shape == (E, N, 4) and w.owner.shape == (E, K) and w.dist.shape == (E, K) and w.stats.shape == (E, 6)
        C2 = ref.cutoff2(sc.cutoff)
        for e in range(E):
            bots, slts = ref.sides(N, K, None if sc.bsel is None else sc.bsel[e], None if sc.ssel is None else sc.ssel[e])
            b, t = np.flatnonzero(w.index[e] >= 0), np.flatnonzero(w.owner[e] >= 0)
            m = len(b)
            assert np.isin(b, bots).all() and np.isin(t, slts).all() and len(t) == m == w.stats[e, 5], (name, e)
            assert len(np.unique(w.index[e, b])) == m and np.array_equal(w.owner[e, w.index[e, b]], b) and np.array_equal(w.index[e, w.owner[e, t]], t), (name, e)
            assert np.array_equal(ref.bits(w.rel[e, b, 2]), ref.bits(w.dist[e, w.index[e, b]])) and (w.rel[e, b, 3] == 1.0).all()
            tx, ty = targets_ref.slots(sc.points[e] if sc.points.ndim == 3 else sc.points)
            d2 = targets_ref.squared(sc.x[e], sc.y[e], tx, ty)[2]
            assert not (d2[b, w.index[e, b]] > C2).any(), (name, e)
            # maximal: no admissible pair between two unmatched entries; without a cutoff the smaller side is used up
            fb, fs = np.setdiff1d(bots, b), np.setdiff1d(slts, t)
            assert (d2[np.ix_(fb, fs)] > C2).all(), (name, e)
            if sc.cutoff is None:
                assert m == min(len(bots), len(slts)), (name, e)
            # the constants of what is not matched
            assert np.isposinf(w.rel[e, fb, 2]).all() and not ref.bits(w.rel[e, fb][:, [0, 1, 3]]).any() and np.isposinf(w.dist[e, fs]).all()
            nob, nos = np.setdiff1d(np.arange(N), bots), np.setdiff1d(np.arange(K), slts)
            assert not ref.bits(w.rel[e, nob]).any() and not ref.bits(w.dist[e, nos]).any()
            assert w.stats[e, 3] <= m and (w.stats[e, 3] >= 1) == (m >= 1) and w.stats[e, 4] <= m
            if m == 0:
                assert not ref.bits(w.stats[e]).any(), (name, e)
            else:
                assert w.stats[e, 1] == w.rel[e, b, 2].max() and abs(float(w.stats[e, 2]) - w.rel[e, b, 2].astype(np.float64).sum()) <= m * 2.0 ** -16


def test_no_scene_is_vacuous(restated):
    for name, (sc, w) in restated.items():
        assert (w.stats[:, 5] > 0).any(), name
    assert [tuple(restated['cloud-%dx%d' % nk][0].x.shape[1:]) + restated['cloud-%dx%d' % nk][0].points.shape[1:2] for nk in AS.CLOUD_SIZES] == AS.CLOUD_SIZES
    assert AS.CLOUD_SIZES == [(1, 1), (7, 5), (5, 7), (65, 63), (257, 255)]


def test_the_chain_takes_every_round(restated):
    sc, w = restated['chain']
    assert sc.x.shape == (1, 64) and sc.points.shape == (64, 2)
    assert w.stats[0, 3] == 64.0 == w.stats[0, 5] and w.index[0].tolist() == list(range(64))


def test_the_tie_scene_ties(restated):
    """Few distinct d2 among 4096 pairs: the index decides nearly every choice, in both envs."""
    sc, w = restated['ties']
    for e in range(2):
        tx, ty = targets_ref.slots(sc.points[e])
        d2 = ref.bits(targets_ref.squared(sc.x[e], sc.y[e], tx, ty)[2])
        assert d2.size == 4096 and len(np.unique(d2)) == 32
        # most kilobots have four slots at the least distance and most slots four kilobots: the least d2 alone decides nothing
        assert ((d2 == d2.min(1, keepdims=True)).sum(1) == 4).sum() == 49 == ((d2 == d2.min(0, keepdims=True)).sum(0) == 4).sum()
    assert w.stats[:, 3].tolist() == [15.0, 15.0] and w.stats[:, 5].tolist() == [64.0, 64.0]


def test_the_cutoff_scene_leaves_both_sides_unmatched(restated):
    sc, w = restated['cutoff']
    nb, ns = (sc.bsel != 0).sum(1), (sc.ssel != 0).sum(1)
    assert sc.x.shape == (2, 333) and sc.points.shape == (2, 129, 2) and sc.bsel.max() > 1 and sc.ssel.max() > 1
    assert (w.stats[:, 5] < np.minimum(nb, ns)).all() and (w.stats[:, 5] > 10).all() and (w.stats[:, 3] >= 3).all()
    free = ref.restate(sc.x, sc.y, sc.th, sc.points, sc.tol, None, sc.bsel, sc.ssel)
    assert (free.stats[:, 5] == np.minimum(nb, ns)).all()


def test_the_pair_scenes(restated):
    sc, w = restated['coincident']
    assert w.index[0].tolist() == [1, 0, 2, -1] and w.owner[0].tolist() == [1, 0, 2] and ref.bits(w.dist[0, 0:1]) == ref.bits(w.dist[0, 2:3])
    sc, w = restated['on-a-slot']
    assert sc.cutoff == 0.0 and w.index[0].tolist() == [-1, 1, -1] and w.owner[0].tolist() == [-1, 1]
    assert w.rel[0, 1].tolist() == [0.0, 0.0, 0.0, 1.0] and w.stats[0].tolist() == [0.0, 0.0, 0.0, 1.0, 1.0, 1.0]
    sc, w = restated['empty-between']
    assert (w.stats[[0, 2], 5] == 30).all() and not ref.bits(w.stats[1]).any() and (w.index[1] == -1).all() and np.isposinf(w.dist[1]).all()
    sc, w = restated['shared']
    assert sc.points.shape == (40, 2)
    assert same(w, ref.restate(sc.x, sc.y, sc.th, np.broadcast_to(sc.points, (3, 40, 2)).copy(), sc.tol))
    sc, w = restated['full']
    assert sc.x.shape == (1, 1024) and sc.points.shape == (1024, 2) and nat.MAX_TARGETS == 1024 == nat.MAX_BOTS and w.stats[0, 5] == 1024 and w.stats[0, 3] > 32


def test_batched_env_target_match_without_a_gpu():
    import torch
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    from tests.oracle_backend import OracleBackend
    pts = np.random.RandomState(1).uniform(-0.5, 0.5, size=(4, 2))

    class Recording(OracleBackend):
        def targets(self, points_m, tol_m, **kw):
            return ('targets', points_m, tol_m, kw)
    a = torch.zeros(3, 16, 2)
    plain = BatchedKilobotsEnv(3, 16, sim_factory=Recording, seed=3, target_obs=(pts, 0.02), target_match=None)
    plain.reset()
    assert plain.targets()[3] == {} and plain.step(a)[3]['targets'][3] == {}
    for bad in ('nearest', 'optimal', 5, ('greedy',), ('greedy', -0.1), ('greedy', float('nan')), ('greedy', 0.1, 2), ('nearest', 0.1), ('greedy', 'a')):
        with pytest.raises(ValueError):
            BatchedKilobotsEnv(3, 16, sim_factory=Recording, target_obs=(pts, 0.02), target_match=bad)
    for match in ('greedy', ('greedy', 0.1)):
        with pytest.raises(ValueError, match='target_obs'):
            BatchedKilobotsEnv(3, 16, sim_factory=Recording, target_match=match)
    for match, kw in (('greedy', {'match': 'greedy'}), (('greedy', 0.25), {'match': 'greedy', 'cutoff_m': 0.25}), (['greedy', 0], {'match': 'greedy', 'cutoff_m': 0.0}),
                      (('greedy', None), {'match': 'greedy'}), (('greedy', float('inf')), {'match': 'greedy'})):
        env = BatchedKilobotsEnv(3, 16, sim_factory=Recording, seed=3, target_obs=(pts, 0.02), target_match=match)
        assert torch.equal(env.reset(), BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3).reset())
        name, points, tol, got = env.targets()
        assert name == 'targets' and tol == 0.02 and got == kw and tuple(points.shape) == (4, 2)
        info = env.step(a)[3]
        assert sorted(info) == ['targets'] and info['targets'][3] == kw
        mask = torch.ones(3, 4, dtype=torch.uint8)
        env.set_targets(slot_select=mask)
        assert env.targets()[3] == dict(kw, slot_select=mask)
        env.set_targets(np.zeros((3, 4, 2)))
        assert env.targets()[3] == kw and tuple(env.targets()[1].shape) == (3, 4, 2)
