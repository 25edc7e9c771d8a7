"""Masked stepping and per-env reset on the device: kb_step_envs and kb_reset_envs through the C ABI against the oracle
(tests/reset_envs_ref.py: envs do not interact, so "run it on all envs and put the unselected ones back" is the exact
reference), against plain kb_step / kb_reset on a twin sim, and byte for byte against the state before the call for the envs
a mask leaves out.  tests/test_reset_envs_cpu.py checks on the oracle that the scenes used here hold contacts before the
masked call and overlap after the resolve step, with a clear status throughout."""
import itertools

import numpy as np
import pytest
import torch

from gym_kilobots_amd import _native as nat
from oracle import oracle as O
from tests import reset_envs_ref as R
from tests import scenes
from tests.gpu_common import OBJ_FIELDS, assert_same, assert_ws_same, cpu, dev

pytestmark = pytest.mark.gpu

BOUND = [n for n in nat.BUFFER_FIELDS if n != 'scratch']      # (scratch is transient by contract)


def make_gpu(case):
    from gym_kilobots_amd.sim import KilobotSim
    c = R.CASES[case]
    return KilobotSim(c['E'], c['N'], c['mode'], c['light'], debug_outputs=True, **R.config_kw(case))


def tensors(g):
    return {n: getattr(g, n) for n in BOUND if getattr(g, n, None) is not None}


def clone(g):
    torch.cuda.synchronize()
    return {n: t.clone() for n, t in tensors(g).items()}


def load(g, snap):
    for n, t in snap.items():
        getattr(g, n).copy_(t)


def assert_rows_equal(g, ref, rows, what):
    """every bound tensor of g but scratch equals `ref` (a clone() or the tensors of another sim) in the envs `rows` selects"""
    torch.cuda.synchronize()
    idx = torch.from_numpy(np.flatnonzero(rows)).cuda()
    got = tensors(g)
    assert set(got) == set(ref)
    for n, t in got.items():
        assert torch.equal(t.index_select(0, idx), ref[n].index_select(0, idx)), '%s: %s differs in envs %s' % (what, n, np.flatnonzero(rows))


def oracle_fields(case):
    """the state arrays that the oracle and the device both keep for a case"""
    c = R.CASES[case]
    f = ['x', 'y', 'theta', 'status']
    if R.takes_actions(case):
        f += ['v', 'w'] + (['acc_v', 'acc_w'] if c['mode'] == O.DRIVE_ACCEL else [])
    else:
        f += ['motor_l', 'motor_r'] + (['pt_threshold', 'pt_update', 'pt_nochange', 'pt_dir'] if c['mode'] == O.DRIVE_PHOTOTAXIS else [])
    if c['light'] != O.LIGHT_NONE:
        f += ['light_x', 'light_y', 'light_vx', 'light_vy']
    if c['kw'].get('num_objects'):
        f += [n for n in OBJ_FIELDS if n not in f]
    if c['kw'].get('allow_sleep'):
        f += ['sleep_time'] + (['osleep'] if c['kw'].get('num_objects') else [])
    if c['kw'].get('sense_radius'):
        f += ['nbr_count']
    return tuple(f)


def give(a):
    return None if a is None else dev(a)


# ---------------------------------------------------------------------------------------------- kb_step_envs
@pytest.mark.parametrize('case', sorted(R.CASES))
def test_step_envs_equals_the_oracle_and_leaves_the_rest_alone(case):
    E = R.CASES[case]['E']
    osim, gsim, twin = R.make_oracle(case), make_gpu(case), make_gpu(case)
    R.prepare(case, [osim, gsim], dev)
    fields = oracle_fields(case)
    assert_same(osim, gsim, 'before the masked call', fields)
    o0, g0 = R.snapshot(osim), clone(gsim)
    for nsub, (name, m) in itertools.product((1, 10), R.masks(E).items()):
        what = '%s, mask %s, %d substeps' % (case, name, nsub)
        sel = m.astype(bool)
        R.restore(osim, o0)
        load(gsim, g0)
        a, la = R.actions(case, 60 + nsub), R.light_action(case, 61 + nsub)

        def go():
            if a is not None:
                osim.set_actions(a)
            osim.step(nsub, light_action=la)
        R.masked(osim, m, go)
        mask = dev(m) if nsub == 10 else dev(sel)           # uint8 and bool alike
        gsim.step(nsub, actions=give(a), light_action=give(la), env_mask=mask)
        assert_same(osim, gsim, what, fields)
        assert_ws_same(osim, gsim, what)
        assert_rows_equal(gsim, g0, ~sel, what)
        moved = cpu((gsim.x != g0['x']).any(1) | (gsim.theta != g0['theta']).any(1))
        assert np.array_equal(moved, sel), what
        if name == 'all':       # every tensor is what a plain kb_step leaves
            load(twin, g0)
            twin.step(nsub, actions=give(a), light_action=give(la))
            assert_rows_equal(gsim, tensors(twin), sel, what + ' against kb_step')
    assert int(cpu(gsim.status).max()) == 0


def test_step_envs_with_nothing_to_do_and_bad_masks():
    gsim = make_gpu('velocity40')
    R.prepare('velocity40', [gsim], dev)
    g0 = clone(gsim)
    m = dev(np.ones(6, np.uint8))
    gsim.step(0, env_mask=m)                                   # no substep, no action: no launch
    assert_rows_equal(gsim, g0, np.ones(6, bool), 'zero substeps')
    for bad in (torch.ones(6, dtype=torch.bool), torch.ones(5, dtype=torch.bool).cuda(), torch.ones(6, dtype=torch.int32).cuda()):
        with pytest.raises(ValueError):
            gsim.step(1, env_mask=bad)
        with pytest.raises(ValueError):
            gsim.reset_envs(bad)


# ---------------------------------------------------------------------------------------------- kb_reset_envs
def poison(case, osim, gsim):
    """what a reset must clear, made visible in every env: a status bit no kernel sets, manifold impulses, object velocities
    and sleep times"""
    osim.status[...] = 64
    gsim.status.fill_(64)
    if R.CASES[case]['kw'].get('num_objects'):
        for n, v in (('ows_acc', 0.5), ('ovx', 0.2), ('ovy', -0.1), ('ow', 0.3)) + ((('osleep', 0.3),) if gsim.osleep is not None else ()):
            getattr(osim, n)[...] = v
            getattr(gsim, n).fill_(v)


def device_reset_envs(case, gsim, m, ep, resolve):
    objects, lights, vel = R.templates(case)
    gsim.reset_envs(dev(m), episode=give(ep), objects=give(objects), lights=give(lights), light_vel=give(vel), **R.reset_kw(case, resolve))


@pytest.mark.parametrize('case', sorted(R.CASES))
def test_reset_envs_equals_the_reference_and_leaves_the_rest_alone(case):
    c = R.CASES[case]
    E, M = c['E'], c['kw'].get('num_objects', 0)
    osim, gsim, twin = R.make_oracle(case), make_gpu(case), make_gpu(case)
    R.prepare(case, [osim, gsim], dev)
    fields = oracle_fields(case)
    o0, g0 = R.snapshot(osim), clone(gsim)
    poison(case, osim, gsim)
    o1, g1 = R.snapshot(osim), clone(gsim)
    objects, lights, vel = R.templates(case)
    words = np.arange(E, dtype=np.int32)
    draw = R.spawn(osim.cfg, z=words, **{k: v for k, v in R.reset_kw(case).items() if k != 'resolve'})
    for (name, m), resolve, counted in itertools.product(R.masks(E).items(), (False, True), (False, True)):
        what = '%s, mask %s, resolve %d, d_episode %d' % (case, name, resolve, counted)
        sel = m.astype(bool)
        ep = words if counted else None
        R.restore(osim, o1)
        load(gsim, g1)
        R.ref_reset_envs(osim, m, episode=ep, objects=objects, lights=lights, light_vel=vel, draw=draw, **R.reset_kw(case, resolve))
        device_reset_envs(case, gsim, m, ep, resolve)
        assert_same(osim, gsim, what, fields)
        assert_ws_same(osim, gsim, what)
        assert_rows_equal(gsim, g1, ~sel, what)
        assert np.array_equal(cpu(gsim.status), np.where(sel, 0, 64)), what          # cleared for the selected envs only
        if not resolve:                # the writes themselves, before a step has touched them
            rows = torch.from_numpy(np.flatnonzero(sel)).cuda()
            assert bool((gsim.ws_cnt.index_select(0, rows) == 0).all()), what
            if M:
                assert torch.equal(torch.stack([gsim.ox, gsim.oy, gsim.otheta], -1).index_select(0, rows), dev(objects).index_select(0, rows)), what
                for t in (gsim.ovx, gsim.ovy, gsim.ow) + ((gsim.osleep,) if gsim.osleep is not None else ()):
                    assert bool((t.index_select(0, rows) == 0).all()), what
                assert bool((gsim.ows_acc.index_select(0, rows) == -1.0).all()), what
            if lights is not None:
                assert torch.equal(torch.stack([gsim.light_x, gsim.light_y, gsim.light_vx, gsim.light_vy], -1).index_select(0, rows),
                                   torch.cat([dev(lights), dev(vel)], -1).index_select(0, rows)), what
        if not counted:                 # without d_episode: the rows of a full kb_reset on a twin, resolve included, bit for bit
            load(twin, g1)
            if M:
                for k, t in enumerate((twin.ox, twin.oy, twin.otheta)):
                    t.copy_(dev(objects[..., k]))
                for t in (twin.ovx, twin.ovy, twin.ow) + ((twin.osleep,) if twin.osleep is not None else ()):
                    t.zero_()
            if lights is not None:
                for k, (t, tv) in enumerate(((twin.light_x, twin.light_vx), (twin.light_y, twin.light_vy))):
                    t.copy_(dev(lights[:, k]))
                    tv.copy_(dev(vel[:, k]))
            twin.reset(**R.reset_kw(case, resolve))
            assert_rows_equal(gsim, tensors(twin), sel, what + ' against kb_reset')
    # a masked reset in mid-run, then five further steps of every env
    R.restore(osim, o0)
    load(gsim, g0)
    m = R.masks(E)['alternating']
    R.ref_reset_envs(osim, m, episode=words, objects=objects, lights=lights, light_vel=vel, draw=draw, **R.reset_kw(case, True))
    device_reset_envs(case, gsim, m, words, True)
    for k in range(5):
        a, la = R.actions(case, 80 + k), R.light_action(case, 90 + k)
        if a is not None:
            osim.set_actions(a)
        osim.step(1, light_action=la)
        gsim.step(1, actions=give(a), light_action=give(la))
        assert_same(osim, gsim, '%s: step %d after the masked reset' % (case, k), fields)
        assert_ws_same(osim, gsim, '%s: step %d after the masked reset' % (case, k))
    assert int(cpu(gsim.status).max()) == 0 and int(osim.status.max()) == 0


def test_reset_envs_of_a_shard_equals_the_rows_of_the_batch():
    from gym_kilobots_amd.sim import KilobotSim
    N = 40
    whole, shard = KilobotSim(8, N), KilobotSim(3, N)
    a = scenes.random_actions(8, N, seed=4).astype(np.float32)
    whole.reset(seed=21, std=0.1, random_theta=True)
    shard.reset(seed=21, std=0.1, random_theta=True, env_offset=3)
    whole.step(5, actions=dev(a))
    shard.step(5, actions=dev(a[3:6]))
    m = np.array([1, 0, 1, 1, 0, 1, 0, 1], np.uint8)
    ep = (np.arange(8) * 3 + 1).astype(np.int32)
    kw = dict(seed=22, mean=(-0.05, 0.02), std=0.1, random_theta=True, random_velocity=True, resolve=True)
    whole.reset_envs(dev(m), episode=dev(ep), **kw)
    shard.reset_envs(dev(m[3:6]), episode=dev(ep[3:6]), env_offset=3, **kw)
    torch.cuda.synchronize()
    rows = tensors(shard)
    for n, t in tensors(whole).items():
        assert torch.equal(t[3:6], rows[n]), n
    assert not torch.equal(whole.x[3], whole.x[5])
    # the mask picked: env 4 (row 1 of the shard) is what the step left
    before = KilobotSim(3, N)
    before.reset(seed=21, std=0.1, random_theta=True, env_offset=3)
    before.step(5, actions=dev(a[3:6]))
    assert torch.equal(before.x[1], shard.x[1]) and not torch.equal(before.x[0], shard.x[0])


# ---------------------------------------------------------------------------------------------- BatchedKilobotsEnv
class _EndsEnvTwoFirst:
    """done_fn: env 2 is done after the first step, nobody else ever (the time limit ends the others)"""

    def __init__(self):
        self.calls = 0

    def __call__(self, prev, actions, obs):
        d = torch.zeros(obs.shape[0], dtype=torch.bool, device=obs.device)
        d[2] = self.calls == 0
        self.calls += 1
        return d


def test_batched_env_auto_reset_on_the_device_equals_the_oracle_backend():
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    E, N = 6, 80
    tmpl = np.array([[[0.3 + 0.01 * e, 0.2, 0.1 * e]] for e in range(E)])
    kw = dict(seed=3, spawn_std=0.12, num_objects=1, auto_reset=True, max_episode_steps=2, object_init=tmpl, env_offset=4)
    g = BatchedKilobotsEnv(E, N, done_fn=_EndsEnvTwoFirst(), **kw)
    o = BatchedKilobotsEnv(E, N, done_fn=_EndsEnvTwoFirst(), sim_factory=R.MaskedOracleBackend, **kw)
    assert type(g.sim).__name__ == 'KilobotSim'
    assert np.array_equal(cpu(g.reset()), o.reset().numpy())
    assert np.array_equal(cpu(g.sim.object_poses()), o.sim.object_poses().numpy())
    dones = np.zeros(E, np.int64)
    for k in range(5):
        a = scenes.random_actions(E, N, seed=30 + k).astype(np.float32)
        og, _, dg, ig = g.step(dev(a))
        oo, _, do, io = o.step(torch.from_numpy(a))
        assert np.array_equal(cpu(og), oo.numpy()), k
        assert np.array_equal(cpu(dg), do.numpy()), k
        assert np.array_equal(cpu(ig['terminal_obs']), io['terminal_obs'].numpy()), k
        assert np.array_equal(cpu(ig['episode_length']), io['episode_length'].numpy()), k
        assert np.array_equal(cpu(g.episode_index), o.episode_index.numpy()), k
        assert np.array_equal(cpu(g.sim.object_poses()), o.sim.object_poses().numpy()), k
        if do.any():        # the new episode is observed, not the end of the old one
            assert not np.array_equal(cpu(og)[do.numpy()], cpu(ig['terminal_obs'])[do.numpy()])
        dones += do.numpy()
    assert dones.tolist() == [2, 2, 3, 2, 2, 2] and cpu(g.episode_index).tolist() == dones.tolist()
    g.close()
