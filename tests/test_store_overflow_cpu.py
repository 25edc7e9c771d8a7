"""The rows of tests/overflow_scenes.py without a GPU: on the oracle alone every row does what its table says, so that the
device test (tests/test_store_overflow_gpu.py) cannot pass on a scene that never overflows.

Slot rows: the status word of every launch; against a twin with room for every contact (ws_slots = 64) from the same start
the slots decide nothing but what is carried over (equal poses after the first substep from a cold store, every stored list
a prefix of the twin's) and the truncation reaches the trajectory (different poses after four substeps); enough kilobots
exceed their slots.  Sleep rows: the swarm falls asleep and is woken again.  Capacity rows: the middle env is flagged in
every launch, the outer envs never are and have contacts of their own.  And the instantiation of kb_step_kernel that every
row's configuration selects, compiled from kb_launch.h on the host: between them the rows reach both pipelines."""
import ctypes as C

import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from gym_kilobots_amd import build as kb_build
from oracle import oracle as O
from tests import overflow_scenes as OS
from tests import scenes
from tests import variant_census as VC

E = OS.E
ROWS = OS.SLOT_ROWS + OS.CAPACITY_ROWS


@pytest.fixture(scope='module')
def selected(tmp_path_factory):
    """{row name: (position in kb_variants, (drive, light, obj, fn, tier, poly, sense, sleep))}"""
    listed, sel = VC.host_census(tmp_path_factory.mktemp('overflow_plan'), [OS.plan_inputs(r) for r in ROWS])
    assert all(status == 0 and index >= 0 for status, index in sel)
    return {r.name: (index, listed[index]) for r, (_, index) in zip(ROWS, sel)}


def test_the_table_has_its_rows():
    names = [r.name for r in ROWS]
    assert len(set(names)) == len(names)
    by = {}
    for r in OS.SLOT_ROWS:
        by.setdefault(r.name.rsplit('-n', 1)[0], set()).add((r.N, r.S))
    assert by['one-wave'] == {(64, 1)} and by['one-wave-dense'] == {(64, 1), (64, 2), (64, 4), (64, 8)}
    assert by['multi-wave'] == {(200, 1), (200, 2)} and by['straddle'] == {(200, 2)}
    assert by['fixed-1024'] == {(1024, 1), (1024, 2)} and by['fixed-1024-lds'] == {(1024, 1)}
    assert by['disc'] == by['sleep'] == {(64, 1), (64, 2), (200, 1), (200, 2)}
    assert [(r.N, r.capacity, r.allow_sleep, r.objects) for r in OS.CAPACITY_ROWS] == \
        [(64, 160, 0, 0), (64, 160, 1, 0), (200, 0, 0, 0), (256, 0, 0, 0), (1024, 0, 0, 0), (64, 200, 0, 1)]
    # the overflowing env is never the last one: what leaves its slice lands in env 2
    assert all(r.spawn[OS.MIDDLE][0] == 'gauss' and [r.spawn[e][0] for e in OS.OUTER] == ['lattice'] * 2 for r in OS.CAPACITY_ROWS)
    # the weaker condition is for two-slot rows on a bare lattice only; every other row has a quarter of its kilobots over the slots
    assert all(r.over == OS.QUARTER for r in OS.SLOT_ROWS if r.name.split('-n')[0] in ('box', 'mixed', 'disc-sleep', 'tier0', 'tier0-sleep'))
    assert all(r.S == 2 and all(kind == 'lattice' for kind, _ in r.spawn) for r in OS.SLOT_ROWS if r.over == OS.FEW)
    assert OS.CONTACTS_SLOT_ROW.solver_modes == OS.ALL_SOLVERS


def test_the_rows_reach_both_pipelines_and_their_sleep_twins(selected):
    """Which kernel each row runs (drive, light, obj, fn, tier, poly, sense, sleep of kb_variant.h)."""
    for r in ROWS:
        print('%-26s instantiation %3d  %s' % (r.name, selected[r.name][0], VC.row_id((OS.plan_inputs(r),) + selected[r.name])))
    slot = {selected[r.name][1] for r in OS.SLOT_ROWS}
    has = lambda **want: any(all(dict(zip(('drive', 'light', 'obj', 'fn', 'tier', 'poly', 'sense', 'sleep'), v))[k] == x for k, x in want.items()) for v in slot)
    V, M = O.DRIVE_VELOCITY, O.DRIVE_MIXED
    for sleep in (0, 1):
        assert has(drive=V, obj=0, fn=0, tier=0, sleep=sleep) and has(drive=V, obj=0, fn=0, tier=2, sleep=sleep)    # sorted bins, 128 / 80 VGPRs
        assert has(drive=V, obj=1, poly=0, sleep=sleep)                                                             # discs
    assert has(drive=V, obj=0, fn=1024, sleep=0)                             # the fixed-size kernel
    assert has(drive=V, obj=1, poly=1, tier=0) and has(drive=V, obj=1, poly=1, tier=1)       # kilobot - polygon contacts, both widths
    assert has(drive=V, obj=1, poly=0, tier=0) and has(drive=V, obj=1, poly=0, tier=1)
    assert has(drive=M, tier=1) and has(drive=M, tier=3)
    cap = {selected[r.name][1] for r in OS.CAPACITY_ROWS}
    assert {(v[2], v[3], v[7]) for v in cap} == {(0, 0, 0), (0, 0, 1), (0, 1024, 0), (1, 0, 0)}


def _launches(r, *sims):
    for k in range(len(r.steps)):
        for s in sims:
            OS.oracle_launch(s, r, k)
        yield k


@pytest.mark.parametrize('r', OS.SLOT_ROWS, ids=OS.row_id)
def test_slot_row_is_flagged_and_enough_kilobots_exceed_their_slots(r):
    o, twin = OS.oracle_sim(r), OS.oracle_sim(r, ws_slots=OS.TWIN_SLOTS)
    want = np.array(r.status)
    flagged = want == 2
    over, full, log = np.zeros(E, np.int64), np.zeros(E, np.int64), []
    for k in _launches(r, o, twin):
        assert not (o.status & 1).any() and not (twin.status & 1).any(), '%s launch %d: contact capacity reached, status %s' % (r.name, k, o.status)
        assert int(twin.status.max()) == 0, 'the twin has room for every contact'
        if k >= r.flag_by:
            assert np.array_equal(o.status, want), '%s launch %d: status %s, the table says %s' % (r.name, k, o.status, want)
        else:
            assert not (o.status & ~want).any()
        if r.steps[k][0] == 1:
            over = np.maximum(over, (twin.ws_cnt > r.S).sum(axis=1))
            full = np.maximum(full, (twin.ws_cnt >= r.S).sum(axis=1))
        log.append('%s/%s' % (OS.counts(o.ws_cnt), OS.counts(twin.ws_cnt)))
    print('%s stored/solved per launch: %s; most owners over S %s, at S or over %s' % (r.name, ' '.join(log), over, full))
    quarter = -(-r.N // 4)
    if r.over == OS.QUARTER:
        assert (over[flagged] >= quarter).all(), '%s: %s of %d kilobots own more than %d contacts' % (r.name, over, r.N, r.S)
    else:
        assert (over[flagged] >= 1).all() and (full[flagged] >= quarter).all(), (r.name, over, full)
    assert not over[~flagged].any()


@pytest.mark.parametrize('r', OS.SLOT_ROWS, ids=OS.row_id)
def test_slots_decide_only_what_is_carried_over(r):
    o, twin = OS.oracle_sim(r), OS.oracle_sim(r, ws_slots=OS.TWIN_SLOTS)
    S = r.S
    # (four substeps; a row whose first kilobots exceed their slots in substep `flag_by` gets four from there)
    for k in range(4 + r.flag_by):
        a = scenes.random_actions(E, r.N, seed=OS.ACTION_SEED + k)
        for s in (o, twin):
            s.set_actions(a)
            s.step(1)
        if k > 0:
            continue
        # from a cold store there is nothing to carry over: the same substep
        for f in ('x', 'y', 'theta'):
            assert np.array_equal(getattr(o, f), getattr(twin, f)), '%s: %s differs after the first substep' % (r.name, f)
        # ... and every owner stored the first min(cnt, S) entries of its list
        assert np.array_equal(o.ws_cnt, np.minimum(twin.ws_cnt, S))
        mine, full = OS.owner_lists(o.ws_cnt, o.ws_key, o.ws_acc), OS.owner_lists(twin.ws_cnt, twin.ws_key, twin.ws_acc)
        for e in range(E):
            for b in range(r.N):
                n = len(mine[e][b][0])
                assert np.array_equal(mine[e][b][0], full[e][b][0][:n]) and np.array_equal(mine[e][b][1], full[e][b][1][:n]), (r.name, e, b)
    flagged = np.array(r.status) == 2
    for e in range(E):
        same = all(np.array_equal(getattr(o, f)[e], getattr(twin, f)[e]) for f in ('x', 'y', 'theta'))
        assert same != bool(flagged[e]), '%s env %d: poses after four substeps %s the twin\'s' % (r.name, e, 'equal' if same else 'differ from')


@pytest.mark.parametrize('r', OS.SLEEP_ROWS, ids=OS.row_id)
def test_sleep_row_falls_asleep_and_is_woken(r):
    o = OS.oracle_sim(r)
    most = np.zeros(E, np.int64)
    for k in _launches(r, o):
        most = np.maximum(most, (o.sleep_time < 0).sum(axis=1))
    end = (o.sleep_time < 0).sum(axis=1)
    print('%s: asleep at most %s, at the end %s' % (r.name, most, end))
    assert (most >= r.N // 2).all(), most
    assert (end <= r.N // 8).all(), end
    assert r.steps[-1] == (10, 'r') and (1, 'r') in r.steps[r.steps.index((10, 'z')):]      # woken by single substeps and a fused launch


@pytest.mark.parametrize('r', OS.CAPACITY_ROWS, ids=OS.row_id)
def test_capacity_row_overflows_in_the_middle_env_only(r):
    o = OS.oracle_sim(r)
    for k in _launches(r, o):
        assert o.status[OS.MIDDLE] & 1, (r.name, k, o.status)
        assert np.array_equal(o.status & 3, np.array(r.status)), (r.name, k, o.status)
        n = OS.counts(o.ws_cnt)
        for e in OS.OUTER:
            assert o.status[e] == 0 and n[e] >= OS.OUTER_MIN_CONTACTS, (r.name, k, e, o.status, n)
    print('%s: capacity %d, stored %s, status %s' % (r.name, o.cap, OS.counts(o.ws_cnt), o.status))
    # the recovery the device test runs: fresh poses forget the contacts, the flag stays
    o.set_poses_m(*OS.recovery_start(r))
    for k in range(OS.RECOVERY_LAUNCHES):
        o.set_actions(OS.recovery_actions(r, k))
        o.step(1)
    assert np.array_equal(o.status & 3, np.array(r.status)) and OS.counts(o.ws_cnt)[OS.MIDDLE] < o.cap // 2


def test_straddle_row_straddles_the_lds_staging_area():
    """stored <= capL < solved in every launch, capL read from the handle kb_create makes of the row (no GPU needed)."""
    r = OS.STRADDLE
    kb_build.build()
    lib = nat.load()
    cfg = nat.default_config(E, r.N, r.mode, O.LIGHT_NONE, **OS.config_kw(r))
    h = C.c_void_p()
    assert lib.kb_create(C.byref(cfg), C.byref(h)) == nat.KB_OK
    capL, cap = lib.kb_lds_staging_entries(h), lib.kb_contact_capacity(h)
    lib.kb_destroy(h)
    o, twin = OS.oracle_sim(r), OS.oracle_sim(r, ws_slots=OS.TWIN_SLOTS)
    assert o.cap == cap
    flagged = np.array(r.status) == 2
    for k in _launches(r, o, twin):
        stored, solved = OS.counts(o.ws_cnt)[flagged], OS.counts(twin.ws_cnt)[flagged]
        print('straddle launch %d: capL %d, stored %s, solved %s' % (k, capL, stored, solved))
        assert (stored <= capL).all() and (solved > capL).all() and (solved <= cap).all(), (k, capL, stored, solved)
