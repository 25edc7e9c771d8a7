"""kb_sense_targets without a GPU: the symbol is exported, bound and declared, the host-side validation answers in the header's
order (arguments before the bound check, so none of it needs a device), the kernel has no private segment and no spill (the
code object's metadata), and the numpy restatement (tests/targets_ref.py) is the intended quantity: in both directions the
winner is a nearest selected entry in float64 up to the rounding of d2, mutual is the fixed point of the two choices, and
the sums are the exact sums of the quantised terms.  The scenes of the GPU tests (tests/targets_scenes.py) hold what they are
there for, checked here on the restatement alone.  BatchedKilobotsEnv checks target_obs at construction."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from tests import targets_ref as ref
from tests import targets_scenes as TS
from tests.host_common import abi_mismatches, Handle, lib, prototypes  # noqa: F401
from tests.sensing_common import kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24      # the unit roundoff of float32


@pytest.fixture(scope='module')
def restated():
    """{name: (scene, restatement)} of every small scene, computed once."""
    return {name: (sc, ref.restate(*sc)) for name, sc in ((n, fn()) for n, fn in TS.SMALL.items())}


def test_symbol_is_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, 'include', 'kilobots_hip.h')).read()
    assert re.search(r'\bint\s+kb_sense_targets\s*\(', hdr) and re.search(r'#define\s+KB_MAX_TARGETS\s+1024\b', hdr)
    assert nat.MAX_TARGETS == 1024
    assert 'kb_sense_targets' in nat.EXPORTS and hasattr(lib, 'kb_sense_targets')
    assert lib.kb_sense_targets.argtypes is not None and len(lib.kb_sense_targets.argtypes) == 13
    assert set(re.findall(r'\b(kb_[a-z_]+)\s*\(', hdr)) == set(nat.EXPORTS)
    ret, params = prototypes()['kb_sense_targets']
    assert ret.strip() == 'int' and len(params) == 13
    assert abi_mismatches(nat.SIGNATURES, lambda name: (getattr(lib, name).restype, getattr(lib, name).argtypes)) == []


def test_check_targets():
    assert nat.check_targets(1, 0) == (1, 0.0) and nat.check_targets(1024, 0.02) == (1024, 0.02) and nat.check_targets(64.0, 1) == (64, 1.0)
    for bad in ((0, 0.02), (1025, 0.02), (-1, 0.02), (8, -0.01), (8, float('inf')), (8, float('nan')), (True, 0.02), (8, True), ('a', 0.02), (8, 'b')):
        with pytest.raises(ValueError):
            nat.check_targets(*bad)


def test_validation_on_an_unbound_handle(lib):
    """Nothing here launches: no pointer is dereferenced on the host.  The errors come in the header's order: NULL sim or
    points, n_targets, tol_m, all outputs NULL, a d_rel off 16 bytes; legal arguments reach the bound check."""
    pts, out, odd, sel = C.c_void_p(0x2000), C.c_void_p(0x1000), C.c_void_p(0x1004), C.c_void_p(0x3000)
    inf, nan = float('inf'), float('nan')
    with Handle(lib) as h:
        bad = [
            ('NULL sim', (None, pts, 8, 0, 0.02, None, None, out, out, out, out, out), b'NULL argument'),
            ('NULL points', (h, None, 8, 0, 0.02, None, None, out, out, out, out, out), b'NULL argument'),
            ('NULL sim before bad n_targets', (None, pts, 0, 0, 0.02, None, None, out, out, out, out, out), b'NULL argument'),
            ('NULL points before bad tol_m', (h, None, 8, 1, -1.0, None, None, out, out, out, out, out), b'NULL argument'),
            ('NULL sim before no output', (None, pts, 8, 0, 0.02, None, None, None, None, None, None, None), b'NULL argument'),
            ('n_targets = 0', (h, pts, 0, 0, 0.02, None, None, out, out, out, out, out), b'KB_MAX_TARGETS'),
            ('n_targets too large', (h, pts, 1025, 1, 0.02, sel, sel, out, None, None, None, None), b'KB_MAX_TARGETS'),
            ('negative n_targets', (h, pts, -4, 0, 0.02, None, None, out, out, out, out, out), b'KB_MAX_TARGETS'),
            ('n_targets before tol_m', (h, pts, 0, 0, -1.0, None, None, out, out, out, out, out), b'KB_MAX_TARGETS'),
            ('n_targets before no output', (h, pts, 1025, 0, 0.02, None, None, None, None, None, None, None), b'KB_MAX_TARGETS'),
            ('n_targets before the alignment', (h, pts, 0, 0, 0.02, None, None, None, odd, None, None, None), b'KB_MAX_TARGETS'),
            ('negative tol_m', (h, pts, 8, 0, -0.01, None, None, out, out, out, out, out), b'tol_m'),
            ('infinite tol_m', (h, pts, 8, 0, inf, None, None, out, out, out, out, out), b'tol_m'),
            ('tol_m that is no number', (h, pts, 8, 1, nan, sel, None, out, out, out, out, out), b'tol_m'),
            ('tol_m before no output', (h, pts, 8, 0, nan, None, None, None, None, None, None, None), b'tol_m'),
            ('tol_m before the alignment', (h, pts, 8, 0, -1.0, None, None, None, odd, None, None, None), b'tol_m'),
            ('no output', (h, pts, 8, 0, 0.02, None, None, None, None, None, None, None), b'all NULL'),
            ('no output, with selections', (h, pts, 1024, 1, 0.0, sel, sel, None, None, None, None, None), b'all NULL'),
            ('d_rel off 16 bytes', (h, pts, 8, 0, 0.02, None, None, out, odd, out, out, out), b'16-byte'),
            ('d_rel alone off 16 bytes', (h, pts, 1, 1, 0.0, sel, sel, None, C.c_void_p(0x1008), None, None, None), b'16-byte'),
        ]
        for what, args, word in bad:
            lib.kb_sense_neighbors(None, 0.07, 8, out, out, out, None)     # (leaves a message that the next call must replace)
            assert lib.kb_sense_targets(*args, None) == nat.KB_EINVAL, what
            msg = lib.kb_last_error()
            assert msg and b'kb_sense_targets' in msg and word in msg, (what, msg)
        # legal arguments reach the bound check: all outputs, each alone (float aligned at the most, d_rel on 16), the limits
        for args in ((pts, 8, 0, 0.02, None, None, out, out, out, out, out), (pts, 1024, 1, 0.0, sel, sel, odd, out, odd, odd, odd),
                     (pts, 1, 0, 0.02, None, None, odd, None, None, None, None), (pts, 5, 1, 1e30, None, sel, None, out, None, None, None),
                     (pts, 5, 0, 0.02, sel, None, None, None, odd, None, None), (pts, 5, 0, 0.02, None, None, None, None, None, odd, None),
                     (odd, 5, 0, 0.02, None, None, None, None, None, None, odd)):
            assert lib.kb_sense_targets(h, *args, None) == nat.KB_ENOTBOUND, args
            assert b'kb_sense_targets' in lib.kb_last_error() and b'kb_bind' in lib.kb_last_error()


def test_kernel_uses_no_scratch_and_spills_nothing(lib):
    """The running bests stay in registers and everything else in LDS: a zero private segment and zero spill counts in the
    metadata of the code object that was linked."""
    found = kernel_metadata('kb_targets_kernel')
    assert len(found) == 1, found
    for name, fields in found:
        for key in ('.private_segment_fixed_size', '.sgpr_spill_count', '.vgpr_spill_count'):
            assert fields[key] == 0, (name, key, fields[key])


def squared_f64(x, y, points):
    """[N, K] float64: the squared distances of the float32 slots (converted in float32, as the definition says) from the
    float32 poses, in double."""
    tx, ty = ref.slots(points)
    ex = tx.astype(np.float64)[None, :] - x.astype(np.float64)[:, None]
    ey = ty.astype(np.float64)[None, :] - y.astype(np.float64)[:, None]
    return ex * ex + ey * ey


def restated_is_intended(sc, w):
    """The properties of the restatement w of the scene sc."""
    E, N = sc.x.shape
    K = sc.points.shape[-2]
    assert w.index.dtype == np.int32 and w.index.shape == (E, N) and w.rel.dtype == np.float32 and w.rel.shape == (E, N, 4)
    assert w.owner.dtype == np.int32 and w.owner.shape == (E, K) and w.dist.dtype == np.float32 and w.dist.shape == (E, K)
    assert w.stats.dtype == np.float32 and w.stats.shape == (E, 6)
    # The float32 d2 = fl(fl(ex * ex) + fl(ey * ey)) with ex = fl(tx - x), ey likewise: each offset carries one rounding, its
    # square two more and the sum a fourth, so d2 = D (1 + t) with |t| <= (1 + U)^4 - 1 =: G for the exact D of the float32
    # inputs (a zero offset is exact).  If o beats b in float32, then D_o (1 - G) <= d2_o <= d2_b <= D_b (1 + G), i.e.
    # D_o - D_b <= G (D_o + D_b): two entries may be taken for one another only if their float64 distances differ by less.
    G = 4.001 * U
    T2 = float(ref.tolerance2(sc.tol))
    for e in range(E):
        bots = np.arange(N) if sc.bsel is None else np.flatnonzero(sc.bsel[e])
        slts = np.arange(K) if sc.ssel is None else np.flatnonzero(sc.ssel[e])
        nob, nos = np.setdiff1d(np.arange(N), bots), np.setdiff1d(np.arange(K), slts)
        assert (w.index[e, nob] == -1).all() and not ref.bits(w.rel[e, nob]).any()
        assert (w.owner[e, nos] == -1).all() and not ref.bits(w.dist[e, nos]).any()
        if len(bots) == 0 or len(slts) == 0:
            assert (w.index[e] == -1).all() and (w.owner[e] == -1).all()
            assert np.isposinf(w.rel[e, bots, 2]).all() and not ref.bits(w.rel[e, bots][:, [0, 1, 3]]).any() and np.isposinf(w.dist[e, slts]).all()
            assert np.isposinf(w.stats[e, :4]).all() and not ref.bits(w.stats[e, 4:]).any()
            continue
        D = squared_f64(sc.x[e], sc.y[e], sc.points[e] if sc.points.ndim == 3 else sc.points)
        t, o = w.index[e, bots], w.owner[e, slts]
        assert np.isin(t, slts).all() and np.isin(o, bots).all()
        Db, Dbest = D[bots, t], D[bots][:, slts].min(1)
        assert (Db - Dbest <= G * (Db + Dbest)).all(), (e, 'kilobot to slot')
        Ds, Dsbest = D[o, slts], D[bots][:, slts].min(0)
        assert (Ds - Dsbest <= G * (Ds + Dsbest)).all(), (e, 'slot to kilobot')
        # the distances are the winners': sqrt and the division round once each, so their square is D (1 + t), |t| < G + 4.1 U
        for got, want in ((w.rel[e, bots, 2], Db), (w.dist[e, slts], Ds)):
            assert (np.abs((got.astype(np.float64) * 25.0) ** 2 - want) <= (G + 4.1 * U) * want).all()
        # the frame: (ahead, left) has the length of the distance, up to the rounding of sine, cosine and six operations
        r = w.rel[e, bots].astype(np.float64)
        assert (np.abs(np.hypot(r[:, 0], r[:, 1]) - r[:, 2]) <= 1e-5 * r[:, 2] + 1e-9).all()
        # mutual is the fixed point of the two choices, and a slot holds at most one kilobot
        mutual = w.owner[e, t] == bots
        assert np.array_equal(w.rel[e, bots, 3], mutual.astype(np.float32))
        assert len(np.unique(t[mutual])) == mutual.sum() <= min(len(bots), len(slts))
        # the sums: exact on the quantised float32 terms, and the float64 sums up to the quantum and the cap
        tx, ty = ref.slots(sc.points[e] if sc.points.ndim == 3 else sc.points)
        _, _, d2 = ref.squared(sc.x[e], sc.y[e], tx, ty)
        for word, d2w, Dw in ((0, d2[bots, t], Db), (2, d2[o, slts], Ds)):
            q = ref.quantised(d2w)
            acc = q.astype(np.float64).sum()
            assert acc < 2.0 ** 53 and acc == int(q.sum(dtype=np.int64))
            assert w.stats[e, word] == (np.float32(acc) / np.float32(65536.0)) / np.float32(625.0)
            if (d2w * 65536.0 < 2.0 ** 40).all():
                assert abs(float(w.stats[e, word]) * 625.0 - Dw.sum()) <= len(Dw) * 2.0 ** -17 + (G + 3 * U) * Dw.sum()
            assert w.stats[e, word + 1] == (w.rel[e, bots, 2] if word == 0 else w.dist[e, slts]).max()
        assert w.stats[e, 4] == (~(d2[o, slts] > np.float32(T2))).sum() and w.stats[e, 5] == (~(d2[bots, t] > np.float32(T2))).sum()


def test_every_scene_is_restated_as_intended(restated):
    assert set(restated) == set(TS.SMALL) and len(TS.SCENES) == len(TS.SMALL) + 1
    for name, (sc, w) in restated.items():
        assert sc.x.dtype == sc.y.dtype == sc.th.dtype == sc.points.dtype == np.float32, name
        restated_is_intended(sc, w)


def test_the_tie_scene_ties_in_both_directions(restated):
    """Env 0: slot 2 is equidistant from kilobots 1 and 3, kilobot 0 from slots 0 and 3, bit for bit; the lower index wins.  Env 1
    holds the same points under reversed indices: the winners are the OTHER kilobot and the other slot."""
    sc, w = restated['ties']
    for e in range(2):
        tx, ty = ref.slots(sc.points[e])
        assert (tx * 8 == np.rint(tx * 8)).all() and (sc.x[e] * 8 == np.rint(sc.x[e] * 8)).all()
        d2 = ref.bits(ref.squared(sc.x[e], sc.y[e], tx, ty)[2])
        tied_bots = (d2 == d2.min(0)[None, :]).sum(0)       # per slot: kilobots at the least distance
        tied_slots = (d2 == d2.min(1)[:, None]).sum(1)      # per kilobot: slots at the least distance
        assert tied_bots.max() == 2 and tied_slots.max() == 2
        assert np.array_equal(w.owner[e], (d2 == d2.min(0)[None, :]).argmax(0)) and np.array_equal(w.index[e], (d2 == d2.min(1)[:, None]).argmax(1))
    assert (w.owner[0, 2], w.index[0, 0]) == (1, 0) and w.dist[0, 2] == np.float32(1.0) / np.float32(25.0)
    # reversed: kilobot b is 6 - b and slot t is 5 - t of env 0; the winners are what were kilobot 3 and slot 3
    assert (w.owner[1, 5 - 2], w.index[1, 6 - 0]) == (6 - 3, 5 - 3)
    assert 6 - w.owner[1, 3] != w.owner[0, 2] and 5 - w.index[1, 6] != w.index[0, 0]


def test_the_pair_scenes(restated):
    sc, w = restated['coincident']
    assert w.index[0, 1] == 1 and w.owner[0, 1] == 1 and w.rel[0, 1].tolist() == [0.0, 0.0, 0.0, 1.0] and ref.bits(w.dist[0, 1:2]).tolist() == [0]
    sc, w = restated['contested']
    assert w.index[0].tolist() == [0, 0, 1] and w.owner[0].tolist() == [0, 2] and w.rel[0, :, 3].tolist() == [1.0, 0.0, 1.0]


def test_the_odd_sizes(restated):
    assert TS.ODD_SIZES == [(1, 1), (7, 5), (5, 7), (333, 129), (64, 1024), (1024, 3)]
    for N, K in TS.ODD_SIZES:
        sc, w = restated['odd-%dx%d' % (N, K)]
        assert sc.x.shape == (2, N) and sc.points.shape == (2, K, 2) and (w.index >= 0).all() and (w.owner >= 0).all()


def test_the_coarse_scenes_tie_across_the_parts_of_a_shared_side(restated):
    """Around 64 and 128 owners, where kb_targets_side shares a side out among the waves: entries whose least d2 is met in
    more than one PART of the other side exist in both directions, and the winner is the lowest index of them all."""
    assert TS.parts_of(64, 1024) == (4, 256) and TS.parts_of(65, 129) == (2, 68) and TS.parts_of(128, 5) == (2, 4) and TS.parts_of(129, 64) == (1, 64)
    for N, K in TS.SHARING_SIZES:
        sc, w = restated['coarse-%dx%d' % (N, K)]
        for e in range(2):
            tx, ty = ref.slots(sc.points[e])
            d2 = ref.bits(ref.squared(sc.x[e], sc.y[e], tx, ty)[2])
            for axis, owners, other, got in ((1, N, K, w.index[e]), (0, K, N, w.owner[e])):
                tied = d2 == d2.min(axis, keepdims=True)
                assert np.array_equal(got, tied.argmax(axis))
                parts, per = TS.parts_of(owners, other)
                part = np.arange(other) // per
                met_in = np.stack([(tied & ((part == p)[None, :] if axis == 1 else (part == p)[:, None])).any(axis) for p in range(parts)]).sum(0)
                assert parts == (4 if owners <= 64 else 2 if owners <= 128 else 1) and (parts == 1 or (met_in >= 2).sum() >= owners // 4), (N, K, e, axis)
                assert parts < 4 or (met_in == 4).any(), (N, K, e, axis)


def test_shared_points_equal_their_copies(restated):
    sc, w = restated['shared']
    assert sc.points.shape == (40, 2)
    per_env = ref.restate(sc.x, sc.y, sc.th, np.broadcast_to(sc.points, (3, 40, 2)).copy(), sc.tol)
    assert all(np.array_equal(ref.bits(a), ref.bits(b)) if a.dtype == np.float32 else np.array_equal(a, b) for a, b in zip(w, per_env))


def test_the_outside_scene_has_both_sides_outside(restated):
    sc, w = restated['outside']
    tx, ty = ref.slots(sc.points)
    assert ((np.abs(tx) > 25.0) | (np.abs(ty) > 18.75)).sum() >= 12
    assert ((np.abs(sc.x) > 25.0) | (np.abs(sc.y) > 18.75)).any(1).all()


def test_the_tolerance_scene_straddles(restated):
    sc, w = restated['tolerance']
    T2 = ref.tolerance2(sc.tol)
    assert sc.tol == TS.TOL and float(T2) == 2.44140625
    tx, ty = ref.slots(sc.points)
    d2 = ref.squared(sc.x[0], sc.y[0], tx, ty)[2]
    assert w.index[0].tolist() == [0, 1, 2] and w.owner[0].tolist() == [0, 1, 2]
    assert d2[0, 0] == T2 and d2[1, 1] == np.nextafter(T2, np.float32(np.inf)) and d2[2, 2] == 0.0
    assert w.stats[0, 4:].tolist() == [2.0, 2.0]
    zero = ref.restate(sc.x, sc.y, sc.th, sc.points, 0.0)
    assert zero.stats[0, 4:].tolist() == [1.0, 1.0] and np.array_equal(ref.bits(zero.stats[0, :4]), ref.bits(w.stats[0, :4]))


def test_the_cap_scene_reaches_the_cap(restated):
    sc, w = restated['cap']
    cap_word = (np.float32(2.0 ** 40) / np.float32(65536.0)) / np.float32(625.0)
    tx, ty = ref.slots(sc.points[0])
    d2 = ref.squared(sc.x[0], sc.y[0], tx, ty)[2]
    assert (d2[:, 1] * np.float32(65536.0) > np.float32(2.0 ** 40)).all() and (d2[:, 0] * np.float32(65536.0) < np.float32(2.0 ** 40)).all()
    assert (w.index[0] == 0).all() and w.stats[0, 0] < 10.0 and w.stats[0, 2] > cap_word and w.stats[0, 2] < cap_word + 1.0
    assert w.stats[1, 0] == ref.sum_word(np.full(5, 2 ** 40, dtype=np.int64)) and w.stats[1, 2] == ref.sum_word(np.full(2, 2 ** 40, dtype=np.int64))
    assert (w.stats[:, 3] > 199.0).all() and np.isfinite(w.stats).all()


def test_the_mask_scene_has_its_empty_envs(restated):
    sc, w = restated['masks']
    nb, ns = (sc.bsel != 0).sum(1), (sc.ssel != 0).sum(1)
    assert nb[2] == nb[4] == 0 and ns[3] == ns[4] == 0 and ns[2] > 100 and nb[3] > 150 and sc.bsel.max() > 1 and sc.ssel.max() > 1
    assert (nb[:2] > 150).all() and (nb[:2] < 270).all() and (ns[:2] > 100).all() and (ns[:2] < 180).all()
    assert np.isposinf(w.stats[2:, :4]).all() and not w.stats[2:, 4:].any() and np.isfinite(w.stats[:2]).all()
    assert np.isposinf(w.dist[2][sc.ssel[2] != 0]).all() and np.isposinf(w.rel[3, sc.bsel[3] != 0, 2]).all()
    assert not ref.bits(w.rel[4]).any() and not ref.bits(w.dist[4]).any()
    everyone = ref.restate(sc.x, sc.y, sc.th, sc.points, sc.tol)
    assert (everyone.index[0] != w.index[0]).any() and (everyone.dist[:2] <= w.dist[:2])[sc.ssel[:2] != 0].all()


def test_the_full_scene_is_the_full_image():
    sc = TS.full()
    assert sc.x.shape == (2, 1024) and sc.points.shape == (1024, 2) and nat.MAX_TARGETS == 1024 == nat.MAX_BOTS
    w = ref.restate_env(sc.x[0], sc.y[0], sc.th[0], sc.points, sc.tol)
    assert 512 < (w.rel[:, 3] == 1.0).sum() < 1024 and 0 < w.stats[5] < 1024


def test_batched_env_target_obs_without_a_gpu():
    import torch
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    from tests.oracle_backend import OracleBackend
    env = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3)
    env.reset()
    a = torch.zeros(3, 16, 2)
    a[..., 0] = 0.01
    assert env.step(a)[3] == {} and env.target_obs is None
    for call in (env.targets, lambda: env.set_targets(np.zeros((4, 2)))):
        with pytest.raises(ValueError, match='target_obs'):
            call()
    pts = np.random.RandomState(1).uniform(-0.5, 0.5, size=(4, 2))
    for bad in (5, (pts,), (pts, 0.02, 1), (pts, -0.01), (pts, float('inf')), (pts[:, :1], 0.02), (np.zeros((0, 2)), 0.02), (np.zeros((1025, 2)), 0.02),
                (np.zeros((2, 4, 2)), 0.02), (np.full((4, 2), np.nan), 0.02), (pts, 'a')):
        with pytest.raises(ValueError):
            BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, target_obs=bad)

    class Recording(OracleBackend):
        def targets(self, points_m, tol_m, **kw):
            return ('targets', points_m, tol_m, kw)
    ok = BatchedKilobotsEnv(3, 16, sim_factory=Recording, seed=3, target_obs=(pts, 0.02))
    assert torch.equal(ok.reset(), BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3).reset())
    name, points, tol, kw = ok.targets()
    assert name == 'targets' and tol == 0.02 and kw == {} and points.dtype == torch.float32 and tuple(points.shape) == (4, 2)
    assert np.array_equal(points.numpy(), pts.astype(np.float32))
    info = ok.step(a)[3]
    assert sorted(info) == ['targets'] and info['targets'][1] is points
    mask = torch.ones(3, 4, dtype=torch.uint8)
    ok.set_targets(slot_select=mask)
    assert ok.targets()[3] == {'slot_select': mask} and ok.targets()[1] is points and ok.step(a)[3]['targets'][3] == {'slot_select': mask}
    per_env = np.random.RandomState(2).uniform(-0.5, 0.5, size=(3, 4, 2))
    ok.set_targets(per_env)
    assert tuple(ok.targets()[1].shape) == (3, 4, 2) and ok.targets()[3] == {} and ok.targets()[2] == 0.02
    for bad in (np.zeros((5, 2)), np.zeros((2, 4, 2)), np.zeros((4, 3))):
        with pytest.raises(ValueError):
            ok.set_targets(bad)
    # a backend without the method says so, as with every other observation
    plain = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3, target_obs=(pts, 0.02))
    with pytest.raises(AttributeError, match='targets'):
        plain.targets()
