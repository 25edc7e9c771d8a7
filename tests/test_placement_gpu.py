"""The packed island placement of the register solver (kb_step_kernel.h, "Placement of the islands on the waves in order of
size"; the rule is stated in tools/placement_model.py) on the device: results never depend on the placement, so every launch
is held bit for bit to the oracle -- state, commands, packed warm-start list, status -- in three single substeps and a fused
launch of ten, with and without the sleep state.

The scenes use the smallest multi-wave shapes, 200 kilobots (two waves) and 256 (four), and are made of touching rectangles
of kilobots 32.5 mm apart (a c x r rectangle is one island of c (r - 1) + r (c - 1) contacts) and single kilobots:

    one slot        every wave closes at one register slot: ncon <= 64 (nw - 1)
    mix             64 nw < ncon < 128 nw in islands below 32 contacts: one-slot waves first, two-slot waves behind them
    big island      one island of more than 64 contacts beside many pairs: the env takes the even split
    out of waves    islands of 24 contacts and pairs that add up to 128 nw: the packing runs out of waves, the env falls back
                    to the even split, and as that overloads a wave too the existing rules decide (cooperative sweep)

What a launch had is read from the DEVICE's packed list (ws_cnt, ws_key): the contact count, the islands, and through the
Python statement of the rule which placement the kernel took and how many one- and two-slot waves it made -- so no scene can
go vacuous.  One case runs the fixed-size instantiation: two envs of the jittered 1024-kilobot lattice, settled for 40
substeps."""
import os
import sys

import numpy as np
import pytest

from tests import scenes
from tests import setup_scenes as SS
from tests import solver_regimes as SR
from tests.gpu_common import make_pair, assert_same, assert_ws_same, cpu, dev
from tests.placement_scenes import E, SCENES, actions, plant

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import placement_model as PM  # noqa: E402

pytestmark = pytest.mark.gpu

SINGLE_LAUNCHES = 3
FIELDS = ('x', 'y', 'theta', 'v', 'w', 'cmd_vx', 'cmd_vy', 'cmd_w')
BIG_ISLAND = 84                 # contacts of the 7 x 7 rectangle
OUT_OF_WAVES_FIRST = 256        # 10 * 24 + 16: exactly 128 nw


def launch_facts(ws_key, ws_cnt, nw):
    """per env (contacts, island sizes, rule, one-slot waves in use, two-slot waves) of the launch behind the lists"""
    out = []
    for e in range(ws_cnt.shape[0]):
        sizes = SS.islands(ws_key[e], ws_cnt[e])
        waves, rule = PM.place(sizes, nw)
        load = PM.loads(sizes, waves, nw)
        out.append((sum(sizes), sizes, rule, sum(1 for c in load if 0 < c <= PM.SLOT), sum(1 for c in load if c > PM.SLOT)))
    return out


def check_scene(s, facts, k, what):
    lo, hi = s.band(s.nw)
    for n, sizes, rule, one, two in facts:
        assert lo <= n <= hi, '%s: %d contacts, the scene is about %d .. %d' % (what, n, lo, hi)
        assert rule == s.first[0], '%s: the placement is %s (islands %s)' % (what, rule, sizes[:8])
        if s.name.startswith('big-island'):
            assert sizes[0] > PM.SLOT, '%s: the largest island has %d contacts' % (what, sizes[0])
        if k == 0:
            if rule == 'packed':
                assert (one, two) == s.first[1:], '%s: %d one-slot and %d two-slot waves' % (what, one, two)
            if s.name.startswith('big-island'):
                assert sizes[0] == BIG_ISLAND, what
            if s.name.startswith('out-of-waves'):
                assert n == OUT_OF_WAVES_FIRST and sizes[0] < PM.CLASSES, '%s: %d contacts' % (what, n)


@pytest.mark.parametrize('allow_sleep', [0, 1], ids=['nosleep', 'sleep'])
@pytest.mark.parametrize('s', SCENES, ids=lambda s: s.name)
def test_scene_is_bit_exact_under_the_packed_placement(s, allow_sleep):
    xy, th = plant(s, seed=77 + s.N)
    osim, gsim = make_pair(E, s.N, xy=xy, th=th, allow_sleep=allow_sleep, solver_mode=0)
    assert gsim.block_threads // SR.LANES == s.nw, 'the handle runs %d waves' % (gsim.block_threads // SR.LANES)
    fields = FIELDS + (('sleep_time',) if allow_sleep else ())
    for k in range(SINGLE_LAUNCHES + 1):
        n = 1 if k < SINGLE_LAUNCHES else SR.FUSED_SUBSTEPS
        a = actions(s, k)
        osim.set_actions(a)
        osim.step(n)
        gsim.step(n, actions=dev(a))
        what = '%s sleep %d, launch %d (%d substeps)' % (s.name, allow_sleep, k, n)
        assert_same(osim, gsim, what, fields)
        assert_ws_same(osim, gsim, what)
        assert np.array_equal(osim.status, cpu(gsim.status)) and int(osim.status.max()) == 0, what
        facts = launch_facts(cpu(gsim.ws_key).view(np.uint32), cpu(gsim.ws_cnt), s.nw)
        print(what, [(f[0], f[2], f[3], f[4]) for f in facts])
        check_scene(s, facts, k, what)


SETTLE = 40


@pytest.mark.parametrize('allow_sleep', [0, 1], ids=['nosleep', 'sleep'])
def test_fixed_size_kernel_on_the_settled_lattice(allow_sleep):
    N, nw = 1024, 8
    xy, th = scenes.lattice_spawn(E, N, seed=21)
    osim, gsim = make_pair(E, N, xy=xy, th=th, allow_sleep=allow_sleep, solver_mode=0)
    assert gsim.block_threads // SR.LANES == nw
    fields = FIELDS + (('sleep_time',) if allow_sleep else ())
    for k in range(-1, SINGLE_LAUNCHES + 1):
        n = SETTLE if k < 0 else 1 if k < SINGLE_LAUNCHES else SR.FUSED_SUBSTEPS
        a = scenes.random_actions(E, N, seed=300 + k)
        osim.set_actions(a)
        osim.step(n, threads=E)
        gsim.step(n, actions=dev(a))
        what = 'lattice sleep %d, launch %d (%d substeps)' % (allow_sleep, k, n)
        assert_same(osim, gsim, what, fields)
        assert_ws_same(osim, gsim, what)
        assert np.array_equal(osim.status, cpu(gsim.status)) and int(osim.status.max()) == 0, what
        facts = launch_facts(cpu(gsim.ws_key).view(np.uint32), cpu(gsim.ws_cnt), nw)
        print(what, [(f[0], f[2], f[3], f[4]) for f in facts])
        for ncon, sizes, rule, one, two in facts:
            # more than one slot's worth of contacts in small islands: the packed rule, with one-slot waves in use
            assert ncon > PM.SLOT and rule == 'packed' and one >= 1, '%s: %d contacts, %s, islands %s' % (what, ncon, rule, sizes[:8])
