"""tests/guarded.py without a GPU: the arena finds a one-byte write on either side of a view and names it; and the contract
that tests/test_state_isolation_gpu.py holds the device to is the oracle's own -- stepping an OracleSim whose dead store
entries are poisoned by the rule of poison_dead_store before every launch gives, bit for bit, the fields and the live
store entries of the plain run.  No row of that comparison is vacuous: every env has live and dead entries."""
import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import overflow_scenes as OV
from tests import solver_regimes as SR
from tests import variant_census as VC


# ---- the arena ------------------------------------------------------------------------------------------------------------
def small_arena():
    arena = G.Arena('cpu', 1 << 20)
    a = arena.take((3, 7), torch.float32, 28, 'a')
    b = arena.take((2, 5000), torch.uint8, 5000, 'b')
    c = arena.take((5,), torch.int32, 4, 'c')
    return arena, a, b, c


def test_views_are_aligned_contiguous_and_banded():
    arena, a, b, c = small_arena()
    assert G.band_bytes(28) == 4096 and G.band_bytes(5000) == 5120 and G.band_bytes(4096) == 4096
    base = arena.buf.data_ptr()
    for t, (name, first, nbytes, front, behind), row in zip((a, b, c), arena.views, (28, 5000, 4)):
        assert t.data_ptr() == base + first and t.data_ptr() % G.ALIGN == 0 and t.is_contiguous()
        assert nbytes == t.numel() * t.element_size()
        assert front >= max(G.MIN_BAND, row) and behind >= max(G.MIN_BAND, row)
        # the bands are canary bytes of the arena's own allocation
        assert first - front >= 0 and first + nbytes + behind <= arena.buf.numel()
        assert bool((arena.buf[first - front:first] == G.CANARY).all()) and bool((arena.buf[first + nbytes:first + nbytes + behind] == G.CANARY).all())
    # no view overlaps another view's bands
    spans = [(first - front, first + nbytes + behind) for _, first, nbytes, front, behind in arena.views]
    assert all(spans[i][1] <= spans[i + 1][0] for i in range(len(spans) - 1))
    assert tuple(a.shape) == (3, 7) and a.dtype == torch.float32 and tuple(b.shape) == (2, 5000) and c.dtype == torch.int32
    assert G.footprint(2 * 5000, 5000) >= spans[1][1] - spans[1][0]


def test_check_passes_on_an_untouched_arena_and_on_writes_inside_the_views():
    arena, a, b, c = small_arena()
    arena.check()
    a.fill_(3.0)
    b.fill_(7)
    c.fill_(-2)
    arena.check()
    G.Arena('cpu', 4096).check()        # nothing taken


@pytest.mark.parametrize('which,side,offset', [('a', 'before', -1), ('a', 'after', 0), ('b', 'before', -5000), ('b', 'after', 4999),
                                               ('c', 'before', -1), ('c', 'after', 0)])
def test_check_reports_buffer_side_and_offset(which, side, offset):
    arena, a, b, c = small_arena()
    name, first, nbytes, _, _ = next(v for v in arena.views if v[0] == which)
    at = first + offset if side == 'before' else first + nbytes + offset
    arena.buf[at] = 0x11
    with pytest.raises(G.GuardError) as err:
        arena.check('launch 3')
    assert str(err.value) == 'launch 3: canary changed: buffer %s, %s, byte offset %d, value 0x11' % (which, side, offset)


def test_check_reports_the_first_changed_byte():
    arena, a, b, c = small_arena()
    _, first, nbytes, _, _ = arena.views[1]
    arena.buf[first + nbytes + 9] = 0
    arena.buf[first - 2] = 1
    with pytest.raises(G.GuardError, match='buffer b, before, byte offset -2, value 0x01'):
        arena.check()


def test_a_full_arena_refuses():
    arena = G.Arena('cpu', 3 * 4096)
    arena.take((16,), torch.uint8, 16)
    with pytest.raises(ValueError):
        arena.take((16,), torch.uint8, 16)


def test_poison_rule_on_tensors():
    cnt = torch.tensor([[1, 2, 0], [0, 0, 0], [3, 3, 3]], dtype=torch.uint8)
    key = torch.full((3, 7), 77, dtype=torch.int32)
    acc = torch.full((3, 7), 0.5)
    G.poison_store_tensors(cnt, key, acc)
    p = torch.arange(7, dtype=torch.int32) % 3
    assert torch.equal(key[0], torch.where(torch.arange(7) < 3, 77, p)) and torch.equal(acc[0, 3:], torch.ones(4)) and bool((acc[0, :3] == 0.5).all())
    assert torch.equal(key[1], p) and bool((acc[1] == 1.0).all())
    assert bool((key[2] == 77).all()) and bool((acc[2] == 0.5).all())        # nine entries owned, seven stored: all live


# ---- the contract on the oracle -------------------------------------------------------------------------------------------
def _census(index):
    row = VC.rows()[index]
    assert row[1] == index
    s = VC.scene(row)
    return (lambda: VC.oracle_sim(s)), [lambda o, step=step: VC.oracle_step(o, step) for step in s.steps], s.fields, None


def _regime(name):
    s = next(s for s in SR.SCENES if s.name == name)

    def make():
        from oracle import oracle as O
        o = O.OracleSim(O.default_config(2, s.N, **SR.config_kw(s, 0)))
        o.set_poses_m(*SR.start(s, 2))
        return o

    def launch(o, k):
        o.set_actions(SR.actions(2, s.N, k))
        o.step(1 if k < s.substeps else SR.FUSED_SUBSTEPS)
    return make, [lambda o, k=k: launch(o, k) for k in range(s.substeps + 1)], ('x', 'y', 'theta', 'v', 'w'), None


def _overflow(name):
    r = next(r for r in OV.SLOT_ROWS + OV.CAPACITY_ROWS if r.name == name)
    flagged = [e for e, st in enumerate(r.status) if st & 1]      # a capacity row: the env that overflows
    return (lambda: OV.oracle_sim(r)), [lambda o, k=k: OV.oracle_launch(o, r, k) for k in range(len(r.steps))], OV.fields(r), flagged


ORACLE_ROWS = {
    'census-001': lambda: _census(1),
    'census-003': lambda: _census(3),
    '200-p014': lambda: _regime('200-p014'),
    'multi-wave-n200-s2': lambda: _overflow('multi-wave-n200-s2'),
    'cap-default-200': lambda: _overflow('cap-default-200'),
}


@pytest.mark.parametrize('name', sorted(ORACLE_ROWS))
def test_the_oracle_never_reads_the_dead_tail_of_the_store(name):
    make, launches, fields, flagged = ORACLE_ROWS[name]()
    plain, poisoned = make(), make()
    cap = plain.cap
    E = plain.ws_cnt.shape[0]
    mixed = np.zeros(E, bool)       # envs that had live AND dead entries after some launch
    for k, launch in enumerate(launches):
        G.poison_oracle_store(poisoned)
        # (the poison is in place: behind the live entries of every env stands the rule's partner with impulse 1)
        n = np.minimum(OV.counts(poisoned.ws_cnt), cap)
        for e in range(E):
            assert np.array_equal(poisoned.ws_key[e, n[e]:], (np.arange(n[e], cap) % plain.ws_cnt.shape[1]).astype(np.uint32))
            assert (poisoned.ws_acc[e, n[e]:] == 1.0).all()
        launch(plain)
        launch(poisoned)
        what = '%s, launch %d' % (name, k)
        for f in tuple(fields) + ('ws_cnt', 'status'):
            a, b = getattr(plain, f), getattr(poisoned, f)
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), '%s: field %s differs' % (what, f)
        n = OV.counts(plain.ws_cnt)
        live = np.arange(cap)[None, :] < np.minimum(n, cap)[:, None]
        assert np.array_equal(plain.ws_key[live], poisoned.ws_key[live]), what + ': live ws_key differs'
        assert np.array_equal(plain.ws_acc[live].view(np.uint32), poisoned.ws_acc[live].view(np.uint32)), what + ': live ws_acc differs'
        mixed |= (n > 0) & (n < cap)
    # (also the flagged env of cap-default-200: it solves more contacts than the capacity, but its owners store at most
    #  ws_slots of them each, 2087 of 2304 entries -- its list is not full)
    assert mixed.all(), '%s: envs %s never had live and dead entries' % (name, np.flatnonzero(~mixed))
    if flagged:
        assert (plain.status[flagged] & 1).all()
