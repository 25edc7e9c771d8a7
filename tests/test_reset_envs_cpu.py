"""Masked stepping and per-env reset (kb_step_envs, kb_reset_envs) without a GPU: the restated spawn against kbo_reset, the
argument checks of the two entry points in their documented order, the per-env episodes of BatchedKilobotsEnv on the oracle
backend, and the conditions that keep the device tests of tests/test_reset_envs_gpu.py from being vacuous."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from gym_kilobots_amd import _native as nat
from gym_kilobots_amd.envs import BatchedKilobotsEnv
from oracle import oracle as O
from tests import reset_envs_ref as R
from tests import scenes
from tests.host_common import lib, word_bits  # noqa: F401


# ---------------------------------------------------------------------------------------------- the restated spawn
@pytest.mark.parametrize('mode', [O.DRIVE_VELOCITY, O.DRIVE_ACCEL, O.DRIVE_MOTORS])
def test_restated_spawn_at_word_zero_is_kbo_reset(mode):
    E, N = 4, 50
    cfg = O.default_config(E, N, mode, allow_sleep=0)
    for (rt, rv), (seed, std) in itertools.product(itertools.product((False, True), repeat=2), ((0, 0.1), (2 ** 40 + 5, 0.6))):
        osim = O.OracleSim(cfg)
        osim.v[...] = 7.0           # (a law that stores no command must not get one)
        kw = dict(seed=seed, mean=(0.05, -0.1), std=std, random_theta=rt, random_velocity=rv, env_offset=3)
        osim.reset(resolve=False, **kw)
        x, y, th, v, w = R.spawn(cfg, z=0, **kw)
        for name, a in (('x', x), ('y', y), ('theta', th)) + ((('v', v), ('w', w)) if mode != O.DRIVE_MOTORS else ()):
            assert np.array_equal(word_bits(getattr(osim, name)), word_bits(a)), (name, rt, rv, seed)
        if std > 0.5:       # (the clip onto the bounds -/+ 0.02 is exercised)
            assert np.abs(osim.y).max() == (np.float32(0.5) * np.float32(1.5) - np.float32(0.02)) * np.float32(25.0)
        if mode == O.DRIVE_MOTORS:
            assert (osim.v == 7.0).all()


def test_other_counter_words_give_other_spawns_in_every_env():
    cfg = O.default_config(5, 40, allow_sleep=0)
    kw = dict(seed=9, std=0.1, random_theta=True, random_velocity=True)
    z0, z1, z2 = (R.spawn(cfg, z=z, **kw) for z in (0, 1, 2))
    for a, b in ((z0, z1), (z0, z2), (z1, z2)):
        for k in range(5):      # x, y, theta, v, w
            assert all(not np.array_equal(a[k][e], b[k][e]) for e in range(5)), k
    # a word per env: env e of the mixed draw is env e of the draw with that word everywhere
    mixed = R.spawn(cfg, z=[0, 1, 2, 1, 0], **kw)
    for e, z in enumerate((z0, z1, z2, z1, z0)):
        assert all(np.array_equal(word_bits(mixed[k][e]), word_bits(z[k][e])) for k in range(5))


# ---------------------------------------------------------------------------------------------- argument checks
def test_argument_errors_in_their_order_on_an_unbound_handle(lib):
    plain, rich = C.c_void_p(), C.c_void_p()
    cfg = nat.default_config(4, 32)
    assert lib.kb_create(C.byref(cfg), C.byref(plain)) == 0
    cfg2 = nat.default_config(4, 32, nat.DRIVE_PHOTOTAXIS, nat.LIGHT_CIRCULAR, num_objects=1)
    assert lib.kb_create(C.byref(cfg2), C.byref(rich)) == 0
    host = (C.c_uint8 * 64)()                      # never read: every call below fails before a launch
    ptr = C.c_void_p(C.addressof(host))
    # kb_step_envs: NULL sim / mask, then the unbound handle, then the checks of kb_step
    assert lib.kb_step_envs(None, ptr, None, None, 1, 0, None) == nat.KB_EINVAL
    assert lib.kb_step_envs(plain, None, None, None, 1, 0, None) == nat.KB_EINVAL
    assert lib.kb_step_envs(plain, None, None, None, -1, 0, None) == nat.KB_EINVAL
    assert lib.kb_step_envs(plain, ptr, None, None, 1, 0, None) == nat.KB_ENOTBOUND
    assert b'kb_step_envs' in lib.kb_last_error() and b'kb_bind' in lib.kb_last_error()
    assert lib.kb_step_envs(plain, ptr, None, None, -1, 0, None) == nat.KB_ENOTBOUND      # (n_substeps < 0 is a check of kb_step: later)
    assert lib.kb_step_envs(rich, ptr, ptr, None, 1, 0, None) == nat.KB_ENOTBOUND         # (so are actions for a law that takes none)
    assert lib.kb_step(plain, None, None, 1, 0, None) == nat.KB_ENOTBOUND                 # kb_step as before
    assert b'kb_step:' in lib.kb_last_error()

    def rp(std=0.1):
        p = nat.KbResetParams()
        p.std = std
        return p

    def init(**kw):
        i = nat.KbEpisodeInit()
        for k in kw:
            setattr(i, k, ptr)
        return i
    good = rp()
    # 1. NULL sim, rp or mask
    assert lib.kb_reset_envs(None, C.byref(good), ptr, None, None) == nat.KB_EINVAL
    assert lib.kb_reset_envs(plain, None, ptr, None, None) == nat.KB_EINVAL
    assert lib.kb_reset_envs(plain, C.byref(good), None, None, None) == nat.KB_EINVAL
    # 2. std, before anything about the handle
    for bad in (-0.1, float('nan')):
        assert lib.kb_reset_envs(plain, C.byref(rp(bad)), ptr, None, None) == nat.KB_EINVAL
        assert b'std' in lib.kb_last_error()
        assert lib.kb_reset_envs(plain, C.byref(rp(bad)), ptr, C.byref(init(d_obj_pose=1)), None) == nat.KB_EINVAL
        assert b'std' in lib.kb_last_error()
    # 3. templates the handle has nothing for, before the unbound handle
    for member in ('d_obj_pose', 'd_light_pos', 'd_light_vel'):
        assert lib.kb_reset_envs(plain, C.byref(good), ptr, C.byref(init(**{member: 1})), None) == nat.KB_EINVAL, member
        assert member.encode() in lib.kb_last_error()
    # 4. the unbound handle
    assert lib.kb_reset_envs(plain, C.byref(good), ptr, None, None) == nat.KB_ENOTBOUND
    assert lib.kb_reset_envs(plain, C.byref(good), ptr, C.byref(init(d_episode=1)), None) == nat.KB_ENOTBOUND
    assert lib.kb_reset_envs(rich, C.byref(good), ptr, C.byref(init(d_obj_pose=1, d_light_pos=1, d_light_vel=1, d_episode=1)), None) == nat.KB_ENOTBOUND
    assert b'kb_reset_envs' in lib.kb_last_error()
    # kb_reset keeps its own order: the unbound handle before std
    assert lib.kb_reset(plain, C.byref(rp(-1.0)), None) == nat.KB_ENOTBOUND
    assert C.sizeof(nat.KbEpisodeInit) == 4 * C.sizeof(C.c_void_p)
    lib.kb_destroy(plain)
    lib.kb_destroy(rich)


def test_episode_init_layout_matches_the_header(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = [n for n, _ in nat.KbEpisodeInit._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "kilobots_hip.h"', 'int main(void) {', 'printf("%zu\\n", sizeof(kb_episode_init));']
    src += ['printf("%%zu\\n", offsetof(kb_episode_init, %s));' % n for n in names] + ['return 0; }']
    c = tmp_path / 'layout.c'
    c.write_text('\n'.join(src))
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-I', os.path.join(root, 'include'), str(c), '-o', exe])
    out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert out == [C.sizeof(nat.KbEpisodeInit)] + [getattr(nat.KbEpisodeInit, n).offset for n in names]


# ---------------------------------------------------------------------------------------------- BatchedKilobotsEnv
E_ENV, N_ENV, LIMIT, STEPS = 6, 40, 3, 8


def _reward(prev, actions, obs):
    return (obs[..., 0] - prev[..., 0]).mean(1)


class _EndsEnvTwo:
    """done_fn: env 2 is done at step 1 (the second step), nobody else ever"""

    def __init__(self):
        self.calls = 0

    def __call__(self, prev, actions, obs):
        d = torch.zeros(obs.shape[0], dtype=torch.bool)
        d[2] = self.calls == 1
        self.calls += 1
        return d


def _env(**kw):
    return BatchedKilobotsEnv(E_ENV, N_ENV, seed=4, spawn_std=0.1, sim_factory=R.MaskedOracleBackend, reward_fn=_reward, env_offset=5,
                              on_status='raise', **kw)


def _actions(k):
    return torch.from_numpy(scenes.random_actions(E_ENV, N_ENV, seed=50 + k).astype(np.float32))


def test_batched_env_ends_and_restarts_single_envs():
    env = _env(max_episode_steps=LIMIT, done_fn=_EndsEnvTwo(), auto_reset=True)
    plain = _env()                                      # the same run with no episode ever ending
    # the reference: an oracle driven by hand
    ref = O.OracleSim(env.sim.cfg)
    key = (4 << 20) + 0
    kw = dict(seed=key, mean=(0.0, 0.0), std=0.1, random_theta=False, random_velocity=False, resolve=True, env_offset=5)
    ref.reset(**kw)
    obs0 = env.reset()
    plain.reset()
    assert np.array_equal(obs0.numpy(), ref.poses_m().astype(np.float32))
    assert not env.episode_index.any()
    steps, index = np.zeros(E_ENV, np.int64), np.zeros(E_ENV, np.int64)
    returns = np.zeros(E_ENV, np.float32)
    fresh = np.ones(E_ENV, bool)            # envs that have not been reset yet: they must equal the plain run
    seen_done = np.zeros(E_ENV, np.int64)
    for k in range(STEPS):
        a = _actions(k)
        before = ref.poses_m().astype(np.float32)
        ref.set_actions(a.numpy())
        ref.step(10)
        terminal = ref.poses_m().astype(np.float32)
        returns = returns + (terminal[..., 0] - before[..., 0]).mean(1, dtype=np.float32)
        steps += 1
        want = steps >= LIMIT
        want[2] |= k == 1
        obs, reward, done, info = env.step(a)
        pobs, _, pdone, pinfo = plain.step(a)
        assert pinfo == {} and not pdone.any()
        assert np.array_equal(done.numpy(), want), k
        assert np.array_equal(info['terminal_obs'].numpy(), terminal), k
        assert np.array_equal(info['episode_length'].numpy()[want], steps[want]), k
        assert np.allclose(info['episode_return'].numpy()[want], returns[want], rtol=1e-5, atol=1e-7), k
        assert np.array_equal(info['terminal_obs'].numpy()[fresh], pobs.numpy()[fresh]), k
        if want.any():
            index[want] += 1
            R.ref_reset_envs(ref, want, episode=index, **kw)
            steps[want], returns[want] = 0, 0.0
            fresh &= ~want
            seen_done += want
        assert np.array_equal(obs.numpy(), ref.poses_m().astype(np.float32)), k
        assert np.array_equal(env.episode_index.numpy(), index), k
        assert np.array_equal(env.episode_steps.numpy(), steps), k
        if want.any():      # the reset envs got new poses, nobody else did
            moved = (obs.numpy() != terminal).any((1, 2))
            assert np.array_equal(moved, want), k
    assert seen_done.min() >= 2 and seen_done[2] == 3 and int(ref.status.max()) == 0


def test_batched_env_reports_done_without_auto_reset():
    env = _env(max_episode_steps=2)
    plain = _env()
    env.reset()
    plain.reset()
    for k in range(3):
        obs, _, done, info = env.step(_actions(k))
        pobs, *_ = plain.step(_actions(k))
        assert torch.equal(obs, pobs) and 'terminal_obs' not in info
        assert bool(done.all()) == (k >= 1) and int(info['episode_length'][0]) == k + 1
    # the caller resets what it likes: here env 1 and env 4
    m = torch.zeros(E_ENV, dtype=torch.bool)
    m[[1, 4]] = True
    before = env.sim.poses()
    after = env.reset_envs(m)
    assert np.array_equal((after != before).any(2).any(1).numpy(), m.numpy())
    assert env.episode_index.tolist() == [0, 1, 0, 0, 1, 0] and env.episode_steps.tolist() == [3, 0, 3, 3, 0, 3]
    assert env.episode_returns[1] == 0 and env.episode_returns[0] != 0


def test_batched_env_defaults_are_what_they_were():
    """No new argument given, or every one given at its default: reset(), step() and the info dict of the env as it was."""
    a = _env()
    b = _env(max_episode_steps=None, done_fn=None, auto_reset=False, object_init=None, light_init=None)
    ref = O.OracleSim(a.sim.cfg)
    ref.reset(seed=(4 << 20), mean=(0.0, 0.0), std=0.1, resolve=True, env_offset=5)
    for env in (a, b):
        assert np.array_equal(env.reset().numpy(), ref.poses_m().astype(np.float32))
    returns = torch.zeros(E_ENV)
    for k in range(3):
        before = torch.from_numpy(ref.poses_m().astype(np.float32))
        ref.set_actions(_actions(k).numpy())
        ref.step(10)
        want = torch.from_numpy(ref.poses_m().astype(np.float32))
        returns += _reward(before, None, want)
        for env in (a, b):
            obs, reward, done, info = env.step(_actions(k))
            assert torch.equal(obs, want) and info == {} and done.dtype == torch.bool and not done.any()
            assert torch.equal(env.episode_returns, returns)
    with pytest.raises(ValueError):
        BatchedKilobotsEnv(2, 8, sim_factory=R.MaskedOracleBackend, object_init=np.zeros((1, 3)))       # no objects
    with pytest.raises(ValueError):
        BatchedKilobotsEnv(2, 8, sim_factory=R.MaskedOracleBackend, light_init=(0.0, 0.0))               # no light
    with pytest.raises(ValueError):
        BatchedKilobotsEnv(2, 8, sim_factory=R.MaskedOracleBackend, max_episode_steps=0)


def test_batched_env_puts_objects_and_lights_in_place():
    tmpl = np.array([[0.5, 0.3, 0.2]])
    light = np.array([0.2, -0.1], np.float32)
    env = BatchedKilobotsEnv(4, 40, nat.DRIVE_PHOTOTAXIS, nat.LIGHT_CIRCULAR, seed=1, spawn_std=0.1, sim_factory=R.MaskedOracleBackend,
                             num_objects=1, object_init=tmpl, light_init=light, max_episode_steps=2, auto_reset=True)
    env.reset()
    want = torch.tensor([np.float32(0.5 * 25.0), np.float32(0.3 * 25.0), np.float32(0.2)])
    for e in range(4):      # (the resolve step moves nothing that does not touch: the object is far from the cloud)
        assert float(env.sim.ox[e, 0]) == float(want[0]) and float(env.sim.otheta[e, 0]) == float(want[2])
        assert float(env.sim.light_x[e]) == float(light[0]) and float(env.sim.light_y[e]) == float(light[1])
    la = torch.full((4, 2), 0.01)
    env.sim.ox += 1.0
    _, _, done, _ = env.step(light_action=la)
    assert not done.any() and float(env.sim.light_x[0]) != float(light[0])
    _, _, done, _ = env.step(light_action=la)
    assert done.all()
    assert float(env.sim.ox[2, 0]) == float(want[0]) and float(env.sim.light_x[3]) == float(light[0]) and float(env.sim.ovx.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------- the device tests are not vacuous
@pytest.mark.parametrize('case', sorted(R.CASES))
def test_scenes_of_the_device_tests_exercise_what_they_claim(case):
    c = R.CASES[case]
    E = c['E']
    osim = R.make_oracle(case)
    R.prepare(case, [osim])
    assert int(osim.status.max()) == 0
    # before the masked call every env holds contacts and is no spawn of either key
    assert (osim.ws_cnt.reshape(E, -1).sum(1) > 0).all()
    for kw, z in ((R.first_reset_kw(case), 0), (R.reset_kw(case), 0), (R.reset_kw(case), np.arange(E))):
        x = R.spawn(osim.cfg, z=z, **{k: v for k, v in kw.items() if k != 'resolve'})[0]
        assert all(not np.array_equal(x[e], osim.x[e]) for e in range(E))
    objects, lights, vel = R.templates(case)
    if objects is not None:
        assert not np.array_equal(objects[..., 0], osim.ox)
    start = R.snapshot(osim)
    for name, m in R.masks(E).items():
        if name not in ('none', 'all'):
            assert 0 < int(m.sum()) < E, name
        sel = m.astype(bool)
        # the masked step: ten substeps with actions, status stays clear
        a, la = R.actions(case, 40), R.light_action(case, 41)

        def go():
            if a is not None:
                osim.set_actions(a)
            osim.step(10, light_action=la)
        R.masked(osim, m, go)
        assert int(osim.status.max()) == 0, name
        assert all(np.array_equal(osim.x[e], start['x'][e]) != bool(sel[e]) for e in range(E)), name
        R.restore(osim, start)
        # the masked reset: the selected envs overlap after the resolve step
        R.ref_reset_envs(osim, m, episode=np.arange(E), objects=objects, lights=lights, light_vel=vel, **R.reset_kw(case))
        assert int(osim.status.max()) == 0, name
        assert (osim.ws_cnt.reshape(E, -1).sum(1)[sel] > 0).all(), name
        assert all(np.array_equal(osim.x[e], start['x'][e]) != bool(sel[e]) for e in range(E)), name
        R.restore(osim, start)
