"""The step kernels where the warm-start store overflows (tests/overflow_scenes.py has the rows, tests/test_store_overflow_cpu.py
shows on the oracle that none is vacuous and which instantiation each selects).

Slot rows (status bit 1, a kilobot with more contacts than ws_slots): the oracle is the specification -- every contact is
solved, the first ws_slots contacts of an owner are stored and warm-started.  Single-substep launches and one fused launch,
after each of them poses, commands, sleep and object state and the packed list (the prefix property on the device) bit
for bit, and the status words.  Capacity rows (status bit 0 in the middle env of three): only the flag is specified for that
env; the envs on both sides of it stay bit-exact, lists included, and after fresh poses all three are.  kb_sense_contacts
reads such stores like any other."""
import numpy as np
import pytest
import torch

from tests import overflow_scenes as OS
from tests import variant_census as VC
from tests.gpu_common import make_pair, assert_same, assert_ws_same, cpu, dev
from tests.sensing_checks import same_contacts as contacts_same, want_contacts as contacts_want

pytestmark = pytest.mark.gpu

E = OS.E
ROWS = OS.SLOT_ROWS + OS.CAPACITY_ROWS


@pytest.fixture(scope='module')
def selected(tmp_path_factory):
    """{row name: position in kb_variants that plan_launch selects}, from the header compiled on the host"""
    _, sel = VC.host_census(tmp_path_factory.mktemp('overflow_plan'), [OS.plan_inputs(r) for r in ROWS])
    assert all(status == 0 for status, _ in sel)
    return {r.name: index for r, (_, index) in zip(ROWS, sel)}


def pair(r, selected, solver_mode=0):
    xy, th = OS.start(r)
    osim, gsim = make_pair(E, r.N, r.mode, xy=xy, th=th, objects=OS.object_start(r), **OS.config_kw(r, solver_mode=solver_mode))
    if r.threads:
        gsim.block_threads = r.threads
    # the kernel the row is there for
    assert gsim.variant_index == selected[r.name], '%s: the handle runs instantiation %d' % (r.name, gsim.variant_index)
    for name, val in OS.state(r).items():
        getattr(osim, name)[...] = val
        getattr(gsim, name).copy_(dev(val))
    return osim, gsim


def launch(osim, gsim, r, k):
    a = OS.actions(r, k)
    osim.set_actions(a)
    osim.step(r.steps[k][0])
    gsim.step(r.steps[k][0], actions=dev(a))


@pytest.mark.parametrize('r,solver_mode', [(r, m) for r in OS.SLOT_ROWS for m in r.solver_modes],
                         ids=lambda v: OS.row_id(v) if hasattr(v, 'name') else 'solver%d' % v)
def test_slot_row_equals_oracle(r, solver_mode, selected):
    osim, gsim = pair(r, selected, solver_mode)
    twin = OS.oracle_sim(r, ws_slots=OS.TWIN_SLOTS) if r is OS.STRADDLE else None
    capL = gsim.lds_staging_entries
    want = np.array(r.status)
    for k in range(len(r.steps)):
        launch(osim, gsim, r, k)
        what = '%s solver %d, launch %d (%d substeps)' % (r.name, solver_mode, k, r.steps[k][0])
        assert_same(osim, gsim, what, OS.fields(r))
        assert_ws_same(osim, gsim, what)
        so, sg = osim.status, cpu(gsim.status)
        assert np.array_equal(so & 3, sg & 3), '%s: status %s on the oracle, %s on the device' % (what, so, sg)
        assert not (sg & 12).any(), '%s: device status %s' % (what, sg)
        if k >= r.flag_by:
            assert np.array_equal(sg & 3, want), '%s: status %s, the table says %s' % (what, sg, want)
        if twin is not None:
            # stored <= capL < solved: the surplus alone sends the substep to the global staging slice
            OS.oracle_launch(twin, r, k)
            flagged = want == 2
            stored, solved = OS.counts(cpu(gsim.ws_cnt))[flagged], OS.counts(twin.ws_cnt)[flagged]
            print('%s: capL %d, stored %s, solved %s' % (what, capL, stored, solved))
            assert (stored <= capL).all() and (solved > capL).all(), (what, capL, stored, solved)
    if r.allow_sleep:
        assert ((cpu(gsim.sleep_time) < 0).sum(axis=1) <= r.N // 8).all(), 'the swarm is awake again at the end'


def assert_envs_same(osim, gsim, envs, what, fields):
    """assert_same and assert_ws_same of tests/test_parity_gpu.py on the envs `envs` only"""
    torch.cuda.synchronize()
    envs = list(envs)
    for f in fields:
        a = getattr(osim, f)
        b = cpu(getattr(gsim, f)).reshape(a.shape)
        assert np.array_equal(a[envs], b[envs]), '%s: field %s differs in envs %s' % (what, f, [e for e in envs if not np.array_equal(a[e], b[e])])
    cnt_o, cnt_g = osim.ws_cnt[envs], cpu(gsim.ws_cnt)[envs]
    assert np.array_equal(cnt_o, cnt_g), what + ': ws_cnt differs'
    key_g, acc_g = cpu(gsim.ws_key).view(np.uint32)[envs], cpu(gsim.ws_acc)[envs]
    assert cpu(gsim.ws_key).shape == osim.ws_key.shape, 'contact capacity differs between oracle and kernel'
    used = np.arange(osim.cap)[None, :] < cnt_o.astype(np.int64).sum(1)[:, None]
    assert np.array_equal(osim.ws_key[envs][used], key_g[used]), what + ': ws_key differs'
    assert np.array_equal(osim.ws_acc[envs][used], acc_g[used]), what + ': ws_acc differs'


@pytest.mark.parametrize('r', OS.CAPACITY_ROWS, ids=OS.row_id)
def test_capacity_row_leaves_the_other_envs_exact_and_recovers(r, selected):
    osim, gsim = pair(r, selected)
    fields = OS.fields(r)
    mid, outer = OS.MIDDLE, list(OS.OUTER)
    for k in range(len(r.steps)):
        launch(osim, gsim, r, k)
        what = '%s, launch %d' % (r.name, k)
        so, sg = osim.status, cpu(gsim.status)
        assert so[mid] & 1 and sg[mid] & 1, '%s: status %s on the oracle, %s on the device' % (what, so, sg)
        assert_envs_same(osim, gsim, outer, what, fields)
        assert not so[outer].any() and not sg[outer].any(), '%s: status %s on the oracle, %s on the device' % (what, so, sg)
    assert (OS.counts(cpu(gsim.ws_cnt))[outer] >= OS.OUTER_MIN_CONTACTS).all()
    if r is OS.CONTACTS_CAPACITY_ROW:
        # kb_sense_contacts on a launch with an overflowed env: the others read their own stores
        exp = contacts_want(gsim, 8)
        got = gsim.contacts(8)
        torch.cuda.synchronize()
        contacts_same(tuple(None if t is None else t[outer] for t in got), tuple(None if t is None else t[outer] for t in exp), r.name)
    # recovery: fresh poses forget the contacts, and all three envs are exact again; the flag stays
    xy, th = OS.recovery_start(r)
    for s in (osim, gsim):
        s.set_poses_m(xy, th)
        if r.objects:
            s.set_objects_m(OS.object_start(r))
    for k in range(OS.RECOVERY_LAUNCHES):
        a = OS.recovery_actions(r, k)
        osim.set_actions(a)
        osim.step(1)
        gsim.step(1, actions=dev(a))
        what = '%s, launch %d after the recovery' % (r.name, k)
        assert_same(osim, gsim, what, fields)
        assert_ws_same(osim, gsim, what)
        so, sg = osim.status, cpu(gsim.status)
        assert np.array_equal(so & 3, sg & 3) and np.array_equal(so & 3, np.array(r.status)), '%s: status %s on the oracle, %s on the device' % (what, so, sg)


def test_contacts_of_a_store_with_truncated_lists():
    """kb_sense_contacts against tests/contacts_ref.py on the device's own store, every owner of which keeps two entries."""
    r = OS.CONTACTS_SLOT_ROW
    xy, th = OS.start(r)
    _, gsim = make_pair(E, r.N, r.mode, xy=xy, th=th, **OS.config_kw(r))
    for k in range(3):
        gsim.step(1, actions=dev(OS.actions(r, k)))
    exp = contacts_want(gsim, 8)
    contacts_same(gsim.contacts(8), exp, r.name)
    assert (cpu(gsim.status) & 3 == 2).all() and int(cpu(gsim.ws_cnt).max()) == r.S and exp[2][..., 0].sum() > 2 * E * r.N
