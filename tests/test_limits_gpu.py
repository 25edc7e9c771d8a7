"""The staging limits that only the device step has (63 partners of one kilobot in one direction, rank 255 in one
(cell, direction) group, 64 kilobots on one fixture, the level table of the cooperative sweep, the candidate list of the
continuous step): an env that runs into one is FLAGGED (status bit 2, bit 3 for the candidates) -- and every other env
of the same launch is still bit-exact against the oracle, which has no such limits.

The three scenes at the top go far past a limit.  The rows of tests/limit_scenes.py pin every limit at its boundary in every
kernel class: the AT scene, with the largest value the model (tests/limits_model.py) calls exact, is bit-exact in every env
with status 0; the OVER scene, one kilobot more, raises exactly the row's bit in the planted env and nothing else, between
the guard bands of tests/guarded.py.  tests/test_limits_cpu.py holds every scene to its claim on the oracle."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import guarded as GD
from tests import limit_scenes as LS
from tests import limits_model as LM
from tests import scenes
from tests.gpu_common import make_pair, cpu, dev, OBJ_FIELDS

pytestmark = pytest.mark.gpu

XB, Y0 = -1.0 + 0.035 * 28, -0.75 + 0.035 * 21 + 0.0175      # a cell boundary in x, the middle of a cell row in y (metres)


def _scene(E, N, env0):
    xy, th = scenes.lattice_spawn(E, N, seed=5, pitch=0.045)
    far = xy[0].copy()
    k = len(env0)
    xy[0, :k] = env0
    # the rest of env 0: the far half of its lattice (nothing near the pile)
    keep = far[np.abs(far[:, 0] - XB) + np.abs(far[:, 1] - Y0) > 0.2]
    xy[0, k:] = keep[:N - k]
    return xy, th


def _check(osim, gsim, steps=3, fields=('x', 'y', 'theta')):
    E = osim.x.shape[0]
    for k in range(steps):
        a = scenes.random_actions(E, osim.x.shape[1], seed=90 + k)
        osim.set_actions(a)
        osim.step(1)
        gsim.step(1, actions=dev(a))
        torch.cuda.synchronize()
        for f in fields:
            assert np.array_equal(getattr(osim, f)[1:], cpu(getattr(gsim, f)).reshape(getattr(osim, f).shape)[1:]), (k, f)
    sg = cpu(gsim.status)
    assert sg[0] & 4, 'env 0 ran into the limit and must say so: status %s' % sg
    assert ((sg[1:] & ~2) == 0).all() and ((osim.status[1:] & 1) == 0).all(), (sg, osim.status)      # the others: nothing dropped


def test_more_than_63_partners_in_one_direction_is_flagged_and_the_other_envs_stay_exact():
    E, N = 3, 128
    pile = [[XB - 0.001, Y0]] + [[XB + 0.001 + 0.00005 * i, Y0 + 0.004 * np.sin(i)] for i in range(66)]
    xy, th = _scene(E, N, np.array(pile))
    osim, gsim = make_pair(E, N, xy=xy, th=th)
    _check(osim, gsim)


def test_more_than_255_contacts_in_one_cell_pair_is_flagged_and_the_other_envs_stay_exact():
    E, N = 3, 128
    west = [[XB - 0.001 - 0.0002 * i, Y0 + 0.003 * np.cos(i)] for i in range(20)]
    east = [[XB + 0.001 + 0.0002 * i, Y0 + 0.003 * np.sin(i)] for i in range(20)]
    xy, th = _scene(E, N, np.array(west + east))
    osim, gsim = make_pair(E, N, xy=xy, th=th, contact_capacity=4096)
    _check(osim, gsim)


def test_more_than_64_kilobots_on_one_fixture_is_flagged_and_the_other_envs_stay_exact():
    E, N = 3, 128
    ring = [[XB + 0.05 * np.cos(0.09 * i), Y0 + 0.05 * np.sin(0.09 * i)] for i in range(70)]     # 70 kilobots inside a disc of 0.075 m
    xy, th = _scene(E, N, np.array(ring))
    objs = np.tile(np.array([[XB, Y0]])[None], (E, 1, 1))
    objs[1:] = [[0.6, 0.4]]
    osim, gsim = make_pair(E, N, xy=xy, th=th, objects=objs, obj_radius=[0.075] * 8, contact_capacity=4096)
    _check(osim, gsim, fields=('x', 'y', 'theta', 'ox', 'oy', 'otheta'))


# ---- the boundary rows -----------------------------------------------------------------------------------------------------
def _device_sim(row, s):
    from gym_kilobots_amd.sim import KilobotSim
    kw = dict(row.kw)
    if s.objects is not None:
        kw['num_objects'] = s.objects.shape[1]

    def make():
        gsim = KilobotSim(LS.E, row.N, row.mode, O.LIGHT_NONE, debug_outputs=True, **kw)
        if row.block_threads:
            gsim.block_threads = row.block_threads
        return gsim
    gsim, arena = GD.guarded_sim(make)
    gsim.set_poses_m(s.xy, s.th)
    if s.objects is not None:
        gsim.set_objects_m(s.objects)
    for name, v in s.state.items():
        getattr(gsim, name).copy_(dev(v))
    return gsim, arena


def _assert_envs_exact(osim, gsim, envs, fields, what):
    """poses, object state and the live entries of the packed store of these envs, bit for bit"""
    for f in fields:
        a = getattr(osim, f)
        b = cpu(getattr(gsim, f)).reshape(a.shape)
        for e in envs:
            assert np.array_equal(a[e].view(np.int32), b[e].view(np.int32)), '%s: env %d, field %s differs in %d elements' % (
                what, e, f, int((a[e].view(np.int32) != b[e].view(np.int32)).sum()))
    cnt = cpu(gsim.ws_cnt)
    key, acc = cpu(gsim.ws_key).view(np.uint32), cpu(gsim.ws_acc)
    assert key.shape == osim.ws_key.shape, 'contact capacity differs between oracle and kernel'
    for e in envs:
        assert np.array_equal(osim.ws_cnt[e], cnt[e]), '%s: env %d, ws_cnt differs' % (what, e)
        n = int(osim.ws_cnt[e].astype(np.int64).sum())
        assert np.array_equal(osim.ws_key[e, :n], key[e, :n]), '%s: env %d, ws_key differs' % (what, e)
        assert np.array_equal(osim.ws_acc[e, :n].view(np.int32), acc[e, :n].view(np.int32)), '%s: env %d, ws_acc differs' % (what, e)


@pytest.mark.parametrize('case', LS.cases(), ids=LS.case_id)
def test_boundary_row(case):
    row, which, slot = case
    lim, shape = LS.row_limits(row.name)
    s = LS.scene(row, which, slot)
    osim = LS.oracle_sim(row, s)
    gsim, arena = _device_sim(row, s)
    assert (gsim.block_threads, gsim.lds_staging_entries, gsim.contact_capacity, gsim.variant_index) == (
        shape.threads, shape.staging, shape.capacity, shape.variant), 'not the handle the row was built for'
    free = LS.oracle_sim(row, s, toi_walls=0) if row.name in LS.NON_INTERACTING and which == 'over' else None
    what = LS.case_id(case)
    fields = ('x', 'y', 'theta') + (OBJ_FIELDS[3:] if s.objects is not None else ())
    osim.step(1)
    gsim.step(1, actions=dev(s.actions))
    torch.cuda.synchronize()
    arena.check(what)
    sg = cpu(gsim.status)
    others = [e for e in range(LS.E) if e != slot]
    assert int(osim.status.max()) == 0, osim.status
    if which == 'at':
        assert (sg == 0).all(), '%s: at the limit nothing may be flagged: status %s' % (what, sg)
        _assert_envs_exact(osim, gsim, range(LS.E), fields, what)
        return
    assert sg[slot] == row.bit, '%s: one past the limit the planted env raises bit value %d and nothing else: status %s' % (what, row.bit, sg)
    assert (sg[others] == 0).all(), '%s: status %s' % (what, sg)
    _assert_envs_exact(osim, gsim, others, fields, what)
    if free is not None:
        # kilobots that touch nobody: whoever found no room in the candidate list skipped the continuous step and is where the
        # oracle without it puts it; everybody else is where the oracle puts it -- and only the overflow may be skipped
        free.step(1)
        pose = lambda sim: np.stack([np.asarray(getattr(sim, f)[slot]).view(np.int32) for f in ('x', 'y', 'theta')], -1)      # noqa: E731
        dev_pose = np.stack([cpu(getattr(gsim, f)).reshape(osim.x.shape)[slot].view(np.int32) for f in ('x', 'y', 'theta')], -1)
        on, off = (dev_pose == pose(osim)).all(-1), (dev_pose == pose(free)).all(-1)
        assert (on | off).all(), '%s: %d kilobots are neither where the continuous step nor where its absence puts them' % (what, int((~(on | off)).sum()))
        skipped = int((~on).sum())
        assert (pose(osim) != pose(free)).any(-1).sum() == lim.candidates + 1        # (every candidate has an event)
        assert skipped == 1, '%s: %d kilobots skipped the continuous step, the list was one short' % (what, skipped)
