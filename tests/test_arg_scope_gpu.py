"""The fixed-size step kernels without objects read their arguments again at the head of every phase (kb_step_kernel.h:
KB_REARG) instead of carrying them from the kernel top.  A stale, mis-scoped or swapped read must not hide, so every argument
of these scenes is off its default: a 1.6 x 1.2 m arena, a kilobot radius of 0.015 m, dt, density and both dampings moved,
7 velocity and 4 position iterations, the continuous step on and off.  All four instantiations run (with and without the
sleep state, with and without IR sensing), 3 envs x 1024 kilobots each -- they exist at no other size.  The launches: one
substep with actions, a fused launch of 3 substeps with actions (the phase heads read again in the second and third), one
substep without an actions tensor, and 3 fused substeps under KB_STEP_NO_DRIVE without one.  After every launch every state
field and the packed warm-start list are compared with the oracle bit for bit.

The oracle runs once per scene (reference()); the test without a GPU shows on it alone that every launch of every scene has
kilobot and wall contacts and ends with status 0."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import oracle as O
from tests import geometry_scenes as GS
from tests.host_common import variants  # noqa: F401

E, N = 3, 1024
W, H, R = 1.6, 1.2, 0.015
VEL_ITERS, POS_ITERS = 7, 4
SENSE_RADIUS = 0.07
CASES = [(sleep, sense, toi) for sleep in (0, 1) for sense in (0, 1) for toi in (0, 1)]
FIELDS = ('x', 'y', 'theta', 'v', 'w', 'cmd_vx', 'cmd_vy', 'cmd_w', 'status')
WS = ('ws_cnt', 'ws_key', 'ws_acc')


def case_id(c):
    return 'sleep%d-sense%d-toi%d' % c


def config_kw(sleep, sense, toi):
    kw = dict(world_width=W, world_height=H, bot_radius=R, allow_sleep=sleep, vel_iters=VEL_ITERS, pos_iters=POS_ITERS, toi_walls=toi,
              sense_radius=SENSE_RADIUS if sense else 0.0)
    kw.update(GS.ALL_BOT)
    return kw


def fields_of(sleep, sense):
    return FIELDS + (('sleep_time',) if sleep else ()) + (('nbr_count',) if sense else ())


@functools.lru_cache(maxsize=None)
def start():
    """Poses [E, N, 2] metres, [E, N]: the lattice of tests/geometry_scenes.py in this arena at this radius, kilobots planted
    against the walls and in the corners; the third env is a second draw."""
    cell, gw, gh = GS.grid(W, H, R)
    g = GS._G('arg-scope', W, H, R, N, 0, cell, gw, gh, 0, 0, 1024, 'phase-scoped arguments')
    (xy, th), (xy2, th2) = GS.start(g, seed=11), GS.start(g, seed=12)
    return np.concatenate([xy, xy2[:1]]), np.concatenate([th, th2[:1]])


def launches():
    """[(substeps, actions or None, flags)]"""
    from tests import scenes
    a0, a1 = scenes.random_actions(E, N, seed=301), scenes.random_actions(E, N, seed=302)
    return [(1, a0, 0), (3, a1, 0), (1, None, 0), (3, None, O.STEP_NO_DRIVE)]


@functools.lru_cache(maxsize=None)
def reference(case):
    """The oracle's state after every launch of the scene: [(fields + warm-start list as a namespace, (kilobot, wall) contacts
    of the last substep -- the least over the envs)]"""
    sleep, sense, toi = case
    osim = O.OracleSim(O.default_config(E, N, O.DRIVE_VELOCITY, O.LIGHT_NONE, **config_kw(sleep, sense, toi)))
    xy, th = start()
    osim.set_poses_m(xy, th)
    out = []
    for n, a, flags in launches():
        if a is not None:
            osim.set_actions(a)
        osim.step(n, flags=flags)
        snap = SimpleNamespace(cap=osim.cap, **{f: np.array(getattr(osim, f)) for f in fields_of(sleep, sense) + WS})
        out.append((snap, GS.oracle_contacts(osim)[:2]))
    return out


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_no_launch_is_vacuous_on_the_oracle(case):
    assert GS.grid(W, H, R)[1:] != GS.grid(2.0, 1.5, GS.R_DEFAULT)[1:] and VEL_ITERS != POS_ITERS and 10 not in (VEL_ITERS, POS_ITERS)
    for k, (snap, (nb, nwall)) in enumerate(reference(case)):
        assert nb > 0 and nwall > 0, (case_id(case), k, nb, nwall)
        assert int(snap.status.max()) == 0, (case_id(case), k, snap.status)
        assert int(snap.ws_cnt.astype(np.int64).sum(1).min()) > 0, (case_id(case), k)
    if case[1]:
        assert int(reference(case)[0][0].nbr_count.max()) > 0


def test_the_moved_arguments_change_the_oracle_result():
    """vel_iters and pos_iters each change the first launch: a kernel that read one where the other is meant cannot pass"""
    base = reference((0, 0, 1))[0][0]
    xy, th = start()
    for swap in (dict(vel_iters=POS_ITERS), dict(pos_iters=VEL_ITERS), dict(bot_radius=GS.R_DEFAULT), dict(world_width=2.0)):
        osim = O.OracleSim(O.default_config(E, N, O.DRIVE_VELOCITY, O.LIGHT_NONE, **dict(config_kw(0, 0, 1), **swap)))
        osim.set_poses_m(xy, th)
        osim.set_actions(launches()[0][1])
        osim.step(1)
        assert not (np.array_equal(osim.x, base.x) and np.array_equal(osim.y, base.y)), swap


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_fixed_size_kernels_read_every_argument_where_it_is_used(case, variants):
    from tests.gpu_common import assert_same, assert_ws_same, cpu, dev
    from gym_kilobots_amd.sim import KilobotSim
    sleep, sense, toi = case
    gsim = KilobotSim(E, N, O.DRIVE_VELOCITY, O.LIGHT_NONE, debug_outputs=True, **config_kw(sleep, sense, toi))
    drive, light, obj, fn, tier, poly, vsense, vsleep = variants[gsim.variant_index]
    assert (obj, fn, vsense, vsleep) == (0, 1024, sense, sleep), variants[gsim.variant_index]
    xy, th = start()
    gsim.set_poses_m(xy, th)
    for k, ((n, a, flags), (snap, _)) in enumerate(zip(launches(), reference(case))):
        gsim.step(n, actions=None if a is None else dev(a), flags=flags)
        what = '%s launch %d (%d substeps, %s actions, flags %d)' % (case_id(case), k, n, 'without' if a is None else 'with', flags)
        assert_same(snap, gsim, what, fields_of(sleep, sense))
        assert_ws_same(snap, gsim, what)
        assert int(cpu(gsim.status).max()) == 0, what
    gsim.close()
