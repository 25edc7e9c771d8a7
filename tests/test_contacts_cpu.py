"""kb_sense_contacts without a GPU: the symbol is exported and bound, the host-side validation answers in the header's order
(arguments before the bound check, so none of it needs a device), the kernels have no private segment and no spill (the code
object's metadata), BatchedKilobotsEnv checks contact_obs at construction -- and the numpy restatement
(tests/contacts_ref.py) on the CPU oracle's store of the four scenes (tests/contacts_scenes.py) is the intended quantity:
symmetric lists, consistent counts, and -- independent of the store's format -- exactly the kilobots and walls that are in
touch on the poses the last substep started from."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from tests import contacts_ref as ref
from tests import contacts_scenes as cs
from tests.host_common import Handle, lib  # noqa: F401
from tests.sensing_common import kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, 'include', 'kilobots_hip.h')).read()
    m = re.search(r'\bint\s+kb_sense_contacts\s*\(([^)]*)\)\s*;', hdr)
    assert m and len(m.group(1).split(',')) == 8
    assert 'kb_sense_contacts' in nat.EXPORTS and hasattr(lib, 'kb_sense_contacts')
    assert lib.kb_sense_contacts.argtypes is not None and len(lib.kb_sense_contacts.argtypes) == 8
    assert lib.kb_sense_contacts.argtypes[2] is C.c_float
    assert re.search(r'#define\s+KB_MAX_CONTACT_SLOTS\s+16\b', hdr) and nat.MAX_CONTACT_SLOTS == 16


def test_validation_on_an_unbound_handle(lib):
    """Nothing here launches: the pointers are never dereferenced on the host.  Every case carries the later errors as well,
    so the message shows which check answered first."""
    P, I, T, O_ = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000), C.c_void_p(0x4000)
    nan, inf = float('nan'), float('inf')
    with Handle(lib) as plain, Handle(lib, num_objects=2) as two:
        bad = [
            # (what, args (sim, k, scale, partner, impulse, touch, obj), a word of the message)
            ('NULL sim', (None, 8, 65536.0, P, I, T, None), b'NULL handle'),
            ('NULL sim before the pairing', (None, 99, nan, P, None, None, None), b'NULL handle'),
            ('partner alone', (two, 8, 65536.0, P, None, T, O_), b'both or neither'),
            ('impulse alone', (two, 8, 65536.0, None, I, T, O_), b'both or neither'),
            ('pairing before k and scale', (plain, 99, nan, P, None, None, O_), b'both or neither'),
            ('k = 0 with lists', (two, 0, 65536.0, P, I, T, O_), b'<= k <='),
            ('k = 17 with lists', (two, 17, 65536.0, P, I, None, None), b'<= k <='),
            ('k = -1 with lists', (two, -1, 65536.0, P, I, None, None), b'<= k <='),
            ('k before scale', (plain, 17, nan, P, I, None, O_), b'<= k <='),
            ('scale NaN', (two, 8, nan, P, I, T, O_), b'scale'),
            ('scale 0', (two, 8, 0.0, P, I, T, O_), b'scale'),
            ('scale negative', (two, 8, -1.0, None, None, T, None), b'scale'),
            ('scale inf', (two, 8, inf, None, None, T, None), b'scale'),
            ('scale before all NULL', (plain, 8, inf, None, None, None, None), b'scale'),
            ('all outputs NULL', (two, 8, 65536.0, None, None, None, None), b'all outputs are NULL'),
            ('all outputs NULL, k ignored', (plain, 99, 65536.0, None, None, None, None), b'all outputs are NULL'),
            ('d_obj without objects', (plain, 8, 65536.0, P, I, T, O_), b'no objects'),
            ('d_obj alone without objects', (plain, 0, 65536.0, None, None, None, O_), b'no objects'),
        ]
        for what, args, word in bad:
            lib.kb_sense_neighbors(None, 0.07, 8, P, P, T, None)     # (leaves a message that the next call must replace)
            assert lib.kb_sense_contacts(*args, None) == nat.KB_EINVAL, what
            msg = lib.kb_last_error()
            assert msg and b'kb_sense_contacts' in msg and word in msg, (what, msg)
        # legal arguments reach the bound check: every NULL combination, k free when no lists are asked for
        legal = [(two, 8, (P, I, T, O_)), (two, 1, (P, I, None, None)), (two, 16, (P, I, T, None)), (two, 4, (P, I, None, O_)),
                 (two, 0, (None, None, T, O_)), (two, 99, (None, None, T, None)), (two, -3, (None, None, None, O_)),
                 (plain, 8, (P, I, T, None)), (plain, 16, (P, I, None, None)), (plain, 0, (None, None, T, None))]
        for h, k, outs in legal:
            assert lib.kb_sense_contacts(h, k, 65536.0, *outs, None) == nat.KB_ENOTBOUND, (k, outs)
            assert b'kb_sense_contacts' in lib.kb_last_error() and b'kb_bind' in lib.kb_last_error()


def test_kernels_use_no_scratch_and_spill_nothing(lib):
    """The sorted lists stay in registers (indexed by constants only), counters and cursors in LDS: every instantiation --
    4, 8 and 16 slots and the aggregate-only form -- has a zero private segment and zero spill counts in the metadata of the
    code object that was linked."""
    found = kernel_metadata('kb_contacts')
    assert len(found) == 4, [n for n, _ in found]
    for name, fields in found:
        for key in ('.private_segment_fixed_size', '.sgpr_spill_count', '.vgpr_spill_count'):
            assert fields[key] == 0, (name, key, fields[key])


def test_batched_env_contact_obs_without_a_gpu():
    import torch
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    from tests.oracle_backend import OracleBackend
    for bad in (-1, 17, 2.5, '8', True, (8,)):
        with pytest.raises(ValueError):
            BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, contact_obs=bad)
    for ok in (0, 8, 16, np.int64(4)):
        assert BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, contact_obs=ok).contact_obs == int(ok)
    env = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3)
    assert env.contact_obs is None
    env.reset()
    a = torch.zeros(3, 16, 2)
    assert env.step(a)[3] == {}
    with pytest.raises(ValueError):
        env.contacts()

    class Recording(OracleBackend):
        def contacts(self, k):
            return ('contacts', k)
    for k in (0, 8):        # k = 0 is an observation like any other: step() asks the sim for it
        env = BatchedKilobotsEnv(3, 16, sim_factory=Recording, seed=3, contact_obs=k)
        env.reset()
        assert env.step(a)[3] == {'contacts': ('contacts', k)} and env.contacts() == ('contacts', k)


# ---- the restatement on the oracle's store ------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def runs():
    """{scene: (scene, store after the resolve step, store after the steps, fixture -> body)} on the CPU oracle, computed once."""
    out = {}
    for name, fn in cs.SCENES.items():
        sc = fn()
        resolved, o = cs.oracle_run(sc)
        out[name] = (sc, resolved, cs.store(o), cs.fixture_body(o.cfg))
    return out


def census(sc, st, fb):
    """Per env of a store: entries, kilobot entries, those with owner > partner, wall entries, object entries, the longest
    list, the largest ws_cnt, kilobots holding both a wall and a kilobot contact, the largest impulse."""
    cnt, key, acc, cap, status = st
    rows = []
    for e in range(sc['E']):
        ents = ref.entries(cnt[e], key[e], acc[e], cap)
        kb = [(a, k) for a, k, _ in ents if k < sc['N']]
        lists = ref.env_lists(cnt[e], key[e], acc[e], cap, sc['N'], fb)
        rows.append(dict(entries=len(ents), kb=len(kb), above=sum(a > k for a, k in kb),
                         walls=sum(ref.KEY_WALL <= k < ref.KEY_WALL + 4 for _, k, _ in ents), objs=sum(k >= ref.KEY_OBJ for _, k, _ in ents),
                         longest=max(len(l) for l in lists), maxcnt=int(cnt[e].max()),
                         both=sum(any(t[3] == 'w' for t in l) and any(t[3] == 'k' for t in l) for l in lists),
                         maximp=max([float(x) for _, _, x in ents] or [0.0]), status=int(status[e])))
    return rows


def test_the_scenes_are_what_they_were_chosen_for(runs):
    """A drifted scene fails here instead of testing nothing."""
    col = lambda rows, k: [r[k] for r in rows]
    for name in runs:
        sc, resolved, stepped, fb = runs[name]
        for st in (resolved, stepped):
            assert col(census(sc, st, fb), 'status') == [0, 0], name
    sc, resolved, stepped, fb = runs['S1']
    r, s = census(sc, resolved, fb), census(sc, stepped, fb)
    assert col(r, 'longest') == [21, 18]            # k = 4, 8 and 16 all truncate
    assert col(r, 'above') == [99, 88] and col(r, 'maximp') == [0.0, 0.0]
    assert col(s, 'walls') == [16, 20] and col(s, 'objs') == [5, 4] and col(s, 'both') == [15, 19]
    assert 0.9 < max(col(s, 'maximp')) < 1.0
    sc, _, stepped, fb = runs['S2']
    s = census(sc, stepped, fb)
    assert col(s, 'entries') == [599, 618] and max(col(s, 'longest')) == 6 and max(col(s, 'maximp')) < 1.3
    sc, _, stepped, fb = runs['S3']
    s = census(sc, stepped, fb)
    assert col(s, 'entries') == [159, 186] and max(col(s, 'longest')) == 2 and col(s, 'above') == [7, 10]
    sc, resolved, _, fb = runs['S4b']
    r = census(sc, resolved, fb)
    assert resolved[3] == 8192 and max(col(r, 'maxcnt')) == 34 and col(r, 'longest') == [43, 45]
    assert col(r, 'entries') == [2053, 1976]        # (about 2000 per env: far beyond what 64 KiB of LDS would hold with the rest)


@pytest.mark.parametrize('name', ['S1', 'S2', 'S3', 'S4b'])
def test_lists_are_symmetric_and_the_counts_agree(runs, name):
    sc, resolved, stepped, fb = runs[name]
    N, M = sc['N'], len(set(fb))
    for what, st in (('resolve', resolved), ('steps', stepped)):
        cnt, key, acc, cap, _ = st
        # k = 16 is the public maximum; the full lists come from env_lists, the truncated ones must be their heads
        partner, impulse, touch, obj = ref.contacts_ref(cnt, key, acc, cap, N, M, fb, 16)
        for e in range(sc['E']):
            lists = ref.env_lists(cnt[e], key[e], acc[e], cap, N, fb)
            pairs = {(i, t[0]): t[2] for i, l in enumerate(lists) for t in l if t[3] == 'k'}
            assert all(pairs.get((j, i)) == b for (i, j), b in pairs.items()), (name, what)       # i lists j iff j lists i, same bits
            nkb = sum(1 for a, k, _ in ref.entries(cnt[e], key[e], acc[e], cap) if k < N and k != a)
            assert touch[e, :, 0].sum() == 2 * nkb == len(pairs), (name, what)
            for i, l in enumerate(lists):
                head = l[:16]
                assert partner[e, i, :len(head)].tolist() == [t[0] for t in head] and (partner[e, i, len(head):] == -1).all()
                assert ref.bits(impulse[e, i, :len(head)]).tolist() == [t[2] for t in head] and not ref.bits(impulse[e, i, len(head):]).any()
                assert touch[e, i, :3].tolist() == [sum(t[3] == c for t in l) for c in 'kwo']
            if M:
                for m in range(M):
                    assert obj[e, m, 0] == sum(t[0] == N + 4 + m for l in lists for t in l)
                assert obj[e, :, 0].sum() == touch[e, :, 2].sum()
        assert (partner is not None) and partner.dtype == np.int32 and touch.dtype == np.float32


R_WU = np.float32(0.0165) * np.float32(25.0)        # a kilobot's radius in world units
BAND = 1e-4                                         # the band keeps the oracle's rounding of the thresholds out of the test, nothing else


@pytest.mark.parametrize('name', ['S2', 'S1'])
def test_lists_are_the_kilobots_and_walls_in_touch_before_the_last_substep(name):
    """The scene one substep at a time; the poses the LAST substep started from decide who is listed: every pair nearer than
    2 r - 1e-4 world units is in both lists and every listed pair is nearer than 2 r + 1e-4; the same for the walls with
    r + 0.01 (b2_polygonRadius) +- 1e-4."""
    from oracle import oracle as O
    sc = cs.SCENES[name]()
    o = O.OracleSim(O.default_config(sc['E'], sc['N'], allow_sleep=0, **sc['kw']))
    cs.place(o, sc)
    o.step(1, flags=cs.STEP_NO_DRIVE)
    o.set_actions(sc['actions'])
    for i in range(10 * sc['steps']):
        x, y = o.x.astype(np.float64), o.y.astype(np.float64)
        o.step(1)
    assert not o.status.any()
    N, fb = sc['N'], cs.fixture_body(o.cfg)
    W, H = 25.0, 18.75
    seen = 0
    for e in range(sc['E']):
        lists = ref.env_lists(o.ws_cnt[e], o.ws_key[e], o.ws_acc[e], o.cap, N, fb)
        d = np.sqrt((x[e][:, None] - x[e][None]) ** 2 + (y[e][:, None] - y[e][None]) ** 2)
        np.fill_diagonal(d, np.inf)
        listed = np.zeros((N, N), bool)
        for i, l in enumerate(lists):
            for t in l:
                if t[3] == 'k':
                    listed[i, t[0]] = True
        assert np.array_equal(listed, listed.T)
        assert listed[d < 2 * float(R_WU) - BAND].all(), name
        assert (d[listed] < 2 * float(R_WU) + BAND).all(), name
        gap = np.stack([x[e] + W, W - x[e], y[e] + H, H - y[e]], -1)     # public order: xmin, xmax, ymin, ymax
        wl = np.zeros((N, 4), bool)
        for i, l in enumerate(lists):
            for t in l:
                if t[3] == 'w':
                    wl[i, t[0] - N] = True
        assert wl[gap < float(R_WU) + 0.01 - BAND].all(), name
        assert (gap[wl] < float(R_WU) + 0.01 + BAND).all(), name
        seen += listed.sum() + wl.sum()
    assert seen > 100
