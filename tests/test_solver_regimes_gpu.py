"""Every contact-count regime of the solver in the step kernels without objects, run on the device against the oracle
(tests/solver_regimes.py has the regimes and the scenes, tests/test_solver_regimes_cpu.py shows that no scene is vacuous).
Per scene and sleep setting: the handle runs the instantiation plan_launch selects, every single-substep launch is
compared bit for bit and classified from the DEVICE's contact counts and staging entries, the set of regimes visited is
the one the table claims, and a fused launch of 10 substeps ends the scene.  Two further cases aim at the cooperative sweep
with the impulses in the global records (R3): replicas of a dense scene on more workgroups than the machine holds at
once, and a sleeping island inside a dense env (contacts that are in the list but in no level of the sweep)."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import solver_regimes as SR
from tests import variant_census as VC
from tests.gpu_common import make_pair, assert_same, assert_ws_same, cpu, dev

pytestmark = pytest.mark.gpu

E = 2


@pytest.fixture(scope='module')
def planned(tmp_path_factory):
    """{(N, capacity, allow_sleep): position in kb_variants that plan_launch selects}, from the header compiled on the host"""
    keys = sorted({(s.N, s.capacity, sl) for s in SR.SCENES + [SR.SLEEP_SCENE] for sl in (0, 1)})
    _, selected = VC.host_census(tmp_path_factory.mktemp('plan'), [SR.plan_inputs(*k) for k in keys])
    assert all(status == 0 for status, _ in selected)
    return {k: index for k, (_, index) in zip(keys, selected)}


def band_of(gsim):
    return (gsim.block_threads // SR.LANES, gsim.lds_staging_entries, gsim.contact_capacity)


@pytest.mark.parametrize('allow_sleep', [0, 1], ids=['nosleep', 'sleep'])
@pytest.mark.parametrize('s', SR.SCENES, ids=SR.scene_id)
def test_scene_is_bit_exact_in_every_regime_it_visits(s, allow_sleep, planned):
    xy, th = SR.start(s, E)
    osim, gsim = make_pair(E, s.N, xy=xy, th=th, **SR.config_kw(s, allow_sleep))
    # the kernel the setting is there for: the sleep state selects another instantiation
    assert gsim.variant_index == planned[s.N, s.capacity, allow_sleep], 'the handle runs instantiation %d' % gsim.variant_index
    assert planned[s.N, s.capacity, 0] != planned[s.N, s.capacity, 1]
    band = band_of(gsim)
    fields = ('x', 'y', 'theta') + (('sleep_time',) if allow_sleep else ())
    seen = []
    for k in range(s.substeps + 1):
        n = 1 if k < s.substeps else SR.FUSED_SUBSTEPS
        a = SR.actions(E, s.N, k)
        osim.set_actions(a)
        osim.step(n)
        gsim.step(n, actions=dev(a))
        what = '%s sleep %d, %s' % (s.name, allow_sleep, 'substep %d' % k if n == 1 else 'fused launch')
        if n == 1:
            seen.append(SR.classify(cpu(gsim.ws_cnt), band))
            what += ' (%s, %s contacts)' % ('/'.join(map(str, seen[-1])), SR.counts(cpu(gsim.ws_cnt)))
        assert_same(osim, gsim, what, fields)
        assert_ws_same(osim, gsim, what)
    print('%s sleep %d band %s:' % (s.name, allow_sleep, band), ' '.join('/'.join(map(str, r)) for r in seen))
    SR.check_visits(s, seen, 'on the device: ')
    assert int(osim.status.max()) == 0 and int(cpu(gsim.status).max()) == 0, (osim.status, cpu(gsim.status))


def test_r3_replicas_on_more_workgroups_than_the_machine_holds():
    """The hand-over of the impulses through the global records (R3) under real residency: 4 distinct envs of the dense
    1024-kilobot scene, tiled to twice the envs that all CUs hold at a time, the default kernel (allow_sleep = 1)."""
    s = SR.REPLICA_SCENE
    D = SR.REPLICA_ENVS
    xy, th = SR.start(s, D)
    from gym_kilobots_amd.sim import KilobotSim
    probe = KilobotSim(D, s.N, **SR.config_kw(s, 1))
    resident = probe.resident_envs_per_cu * torch.cuda.get_device_properties(probe.device).multi_processor_count
    probe.close()
    Eg = min(D * -(-2 * resident // D), 2048)
    reps = Eg // D
    assert Eg > resident, 'the launch must not fit the machine at once: %d envs, %d resident' % (Eg, resident)
    gsim = KilobotSim(Eg, s.N, **SR.config_kw(s, 1))
    gsim.set_poses_m(np.tile(xy, (reps, 1, 1)), np.tile(th, (reps, 1)))
    osim = O.OracleSim(O.default_config(D, s.N, **SR.config_kw(s, 1)))
    osim.set_poses_m(xy, th)
    band = band_of(gsim)
    first = slice(0, D)
    for k in range(s.substeps):
        a = SR.actions(D, s.N, k)
        osim.set_actions(a)
        osim.step(1, threads=D)
        gsim.step(1, actions=dev(np.tile(a, (reps, 1, 1))))
        torch.cuda.synchronize()
        cnt = cpu(gsim.ws_cnt)
        regimes = set(SR.classify(cnt, band))
        assert regimes == {'R3'}, 'substep %d: %s (contacts %d .. %d)' % (k, regimes, SR.counts(cnt).min(), SR.counts(cnt).max())
        for f in ('x', 'y', 'theta', 'ws_cnt'):
            t = getattr(gsim, f)
            t = t.reshape(reps, D, -1)
            assert torch.equal(t, t[:1].expand_as(t)), 'substep %d: replicas differ in %s' % (k, f)
            assert np.array_equal(getattr(osim, f), cpu(getattr(gsim, f)[first])), 'substep %d: %s differs from the oracle' % (k, f)
        used = np.arange(osim.cap)[None, :] < SR.counts(osim.ws_cnt)[:, None]
        assert np.array_equal(osim.ws_acc[used], cpu(gsim.ws_acc[first])[used]), 'substep %d: impulses differ from the oracle' % k
        acc = gsim.ws_acc.reshape(reps, D, -1)
        assert torch.equal(torch.where(dev(used)[None], acc, 0.0), torch.where(dev(used)[None], acc[:1], 0.0).expand_as(acc)), \
            'substep %d: replicas differ in the impulses' % k
    assert int(osim.status.max()) == 0 and int(gsim.status.max().item()) == 0
    print('replicas: %d envs on %d resident, band %s' % (Eg, resident, band))


def test_sleeping_island_inside_a_dense_env(planned):
    """64 kilobots asleep with 112 contacts among them beside a dense awake crowd: their contacts are in the list (and
    count for the regime) but in no level of the cooperative sweep, in R3, R2 and R1."""
    s = SR.SLEEP_SCENE
    xy, th, sleep_time = SR.sleeping_island_start(E)
    osim, gsim = make_pair(E, s.N, xy=xy, th=th, **SR.config_kw(s, 1))
    assert gsim.variant_index == planned[s.N, s.capacity, 1]
    osim.sleep_time[...] = sleep_time
    gsim.sleep_time.copy_(dev(sleep_time))
    band = band_of(gsim)
    seen, resting = [], None
    S, C = SR.SLEEPERS, SR.SLEEPER_CONTACTS
    for k in range(s.substeps + 1):
        n = 1 if k < s.substeps else SR.FUSED_SUBSTEPS
        a = SR.sleeping_island_actions(E, k)
        osim.set_actions(a)
        osim.step(n)
        gsim.step(n, actions=dev(a))
        what = 'sleeping island, launch %d' % k
        assert_same(osim, gsim, what, ('x', 'y', 'theta', 'sleep_time'))
        assert_ws_same(osim, gsim, what)
        cnt = cpu(gsim.ws_cnt)
        assert (SR.sleeper_entries(cnt) == C).all(), '%s: the sleepers own %s contacts' % (what, SR.sleeper_entries(cnt))
        st = cpu(gsim.sleep_time)
        assert (st[:, :S] < 0).all() and (st[:, S:] >= 0).all(), what
        held = (cpu(gsim.ws_key)[:, :C].copy(), cpu(gsim.ws_acc)[:, :C].copy())
        if resting is None:
            resting = held
        assert np.array_equal(resting[0], held[0]) and np.array_equal(resting[1], held[1]), '%s: the sleepers\' entries changed' % what
        if n == 1:
            seen.append(SR.classify(cnt, band))
    print('sleeping island band %s:' % (band,), ' '.join('/'.join(map(str, r)) for r in seen))
    SR.check_visits(s, seen, 'on the device: ')
    assert np.array_equal(cpu(gsim.x)[:, :S], (xy[:, :S, 0] * 25.0).astype(np.float32))
    assert int(osim.status.max()) == 0 and int(cpu(gsim.status).max()) == 0
