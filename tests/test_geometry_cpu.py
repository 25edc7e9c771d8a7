"""The rows of tests/geometry_scenes.py without a GPU: the guard against a vacuous device test.

Grid and launch shape: the grid of every geometry row by kb_create's fp32 expressions restated in numpy, plan_launch through
the header compiled on the host, and kb_create of the library through its ABI -- each row runs the cell size, the grid,
the hashed or direct bins, the islMin placement and the kernel it is in the table for, and the table cannot be thinned
without a test failing.  Containment: wherever islMin lies, its NB words end inside the LDS image, for every cell count
(the fixed-size kernel places it by ldsb::binE, not by the plan's offset).  Oracle: every geometry row has the contacts, the
sleepers and the waking it is there for with status 0, and every constants row moves the trajectory of the bodies its
constant acts on away from the default-constants run of the same scene."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from oracle import oracle as O
from tests import geometry_scenes as GS
from tests.host_common import compile_host, lib, plans_of, word_bits  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY_OBJ = 0x20000

# every cell count 1 .. 8192 with the sleep state: the fixed-size kernel (1024 kilobots) and the generic kernels of every
# swarm size (kb_create's width, and every other width kb_set_block_threads accepts for the swarm at the cell counts of the
# table); prints up to five violations, then their number, the number of plans per islMin placement, the plans of the
# fixed-size kernel and the plans that place islMin behind the image at a width other than kb_create's
CONTAINMENT_PROGRAM = r'''
#include <cstdio>
#include "kb_launch.h"
using namespace kb;
static long bad = 0, plans[4] = {0, 0, 0, 0}, fixed = 0, behind_at_a_second_width = 0;
static void check(int N, int ncell, int threads) {
    const Plan p = plan_launch({N, 0, 0, false, KB_DRIVE_VELOCITY, KB_LIGHT_NONE, false, true, ncell, 0, threads});
    if (p.status != KB_OK) return;
    const int NP = (N + 3) & ~3, NB = NP + KB_MAX_OBJECTS + 4;
    const bool hashed = p.hmask != 0;
    const int branch = p.islmin_off == ldsb::binE(NB, NP, hashed, p.capL) ? 1 : p.islmin_off == ldsb::con32(NB, NP, hashed, p.capL, 0) ? 2
                     : p.islmin_off == ldsb::total(NB, NP, hashed, p.capL, p.nhead, p.threads / 64) ? 3 : 0;
    ++plans[branch];
    if (threads && branch == 3 && plan_launch({N, 0, 0, false, KB_DRIVE_VELOCITY, KB_LIGHT_NONE, false, true, ncell, 0, 0}).threads != threads) ++behind_at_a_second_width;
    fixed += p.variant.fn != 0;
    // the fixed-size kernel: kb_step_kernel.h takes ldsb::binE(NB, NP, false, capL) for islMin
    const int at = p.variant.fn ? ldsb::binE(NB, NP, false, p.capL) : p.islmin_off;
    const bool ok = branch != 0 && at >= 0 && at % 4 == 0 && at + 4 * NB <= p.lds_total && p.lds_total <= LDS_CU
        && (!p.variant.fn || (p.capL == ldsb::CAPL && !hashed));
    if (!ok && ++bad <= 5) printf("N %d ncell %d threads %d: islMin at %d (+ %d) in an image of %d\n", N, ncell, p.threads, at, 4 * NB, p.lds_total);
}
int main(int argc, char **argv) {
    for (int ncell = 1; ncell <= MAX_CELLS_; ++ncell) {
        check(1024, ncell, 0);
        for (int N = 1; N < 1024; ++N) check(N, ncell, 0);
    }
    int ncell;
    while (scanf("%d", &ncell) == 1)
        for (int N = 1; N <= 1024; ++N)
            for (int T = 64; T <= 64 * MAX_WAVES; T += 64) check(N, ncell, T);
    printf("%ld %ld %ld %ld %ld %ld %ld\n", bad, plans[0], plans[1], plans[2], plans[3], fixed, behind_at_a_second_width);
    return 0;
}
'''.replace('MAX_CELLS_', str(GS.MAX_CELLS))


@pytest.fixture(scope='module')
def planned(tmp_path_factory):
    return plans_of(tmp_path_factory.mktemp('geometry'), GS.GEOMETRY)


def test_rows_claim_the_grid_kb_create_derives():
    for g in GS.GEOMETRY:
        assert GS.grid(g.W, g.H, g.r) == (g.cell, g.gw, g.gh), g.name
        assert 2.0 * g.r * GS.WORLD_SCALE <= g.cell and g.gw * g.gh <= GS.MAX_CELLS, g.name
    assert GS.grid(2.0, 1.5, GS.R_DEFAULT) == (0.875, 58, 43)              # the arena of every other suite
    for c in GS.CONSTANTS:
        assert (c.cell, c.gw, c.gh) == (0.875, 58, 43), c.name


def test_rows_claim_the_plan_of_the_header(planned):
    for g, (status, cap, capL, nhead, hmask, threads, lds_total, islmin_off, botlaw_off, tier), variant, index, branch, inside in planned:
        drive, light, obj, fn, vtier, poly, sense, sleep = variant
        what = '%s: plan hashed %d (nhead %d) branch %d fn %d sleep %d threads %d lds %d' % (g.name, hmask != 0, nhead, branch, fn, sleep, threads, lds_total)
        assert (hmask != 0) == bool(g.hashed), what
        assert nhead == (hmask + 1 if hmask else g.gw * g.gh), what
        assert fn == g.fn and sleep == g.sleep, what
        if g.family == 'bins' and g.sleep:
            assert branch == g.branch, what
        else:                                            # no sleep state or not a sorted-bin kernel: the row claims no placement
            assert g.branch == 0 and (branch == 0 or g.family == 'bins'), what
        assert inside == 1, what
        # (the mixed kernels are instantiations of the kernel with objects: the head table in front of the manifold records)
        assert obj == (g.family != 'bins') and drive ==(O.DRIVE_MIXED if g.family == 'mixed' else O.DRIVE_VELOCITY), what
        if g.family != 'bins':
            assert threads == 64, what                   # 96 kilobots with objects or mixed laws: one wave


def test_the_library_plans_what_the_header_plans(lib, planned):
    h = C.c_void_p()
    for g, (status, cap, capL, nhead, hmask, threads, lds_total, *_), variant, index, branch, inside in planned:
        cfg = nat.default_config(1, g.N, O.DRIVE_MIXED if g.family == 'mixed' else O.DRIVE_VELOCITY, O.LIGHT_NONE, **GS.config_kw(g))
        assert lib.kb_create(C.byref(cfg), C.byref(h)) == nat.KB_OK, (g.name, lib.kb_last_error())
        got = (lib.kb_contact_capacity(h), lib.kb_lds_staging_entries(h), lib.kb_block_threads(h), lib.kb_lds_bytes(h), lib.kb_variant_index(h))
        lib.kb_destroy(h)
        assert got == (cap, capL, threads, lds_total, index), g.name


def test_the_table_covers_what_it_is_there_for():
    for what, holds, least in GS.COVERAGE:
        n = sum(1 for g in GS.GEOMETRY if holds(g))
        assert n >= least, '%s: %d rows, at least %d wanted' % (what, n, least)
    arenas = {(g.W, g.H, g.r) for g in GS.GEOMETRY if g.fn == 1024}
    assert len(arenas) >= GS.FIXED_ARENAS, arenas
    names = [g.name for g in GS.GEOMETRY] + [c.name for c in GS.CONSTANTS]
    assert len(set(names)) == len(names)
    # the constants table: every kilobot constant on all three kernels, every object constant on the objects kernel, each
    # with the continuous step off and on
    for toi in (0, 1):
        for kernel in GS.CONSTANT_KERNELS:
            have = {c.constant for c in GS.CONSTANTS if c.kernel == kernel and c.toi == toi}
            want = {'default', 'all'} | {n for n, _, _ in GS.BOT_CONSTANTS} | ({n for n, _, _ in GS.OBJ_CONSTANTS} if kernel == 'objects' else set())
            assert have == want, (kernel, toi, have ^ want)
    moved = set()
    for n, c, _ in GS.BOT_CONSTANTS + GS.OBJ_CONSTANTS:
        moved |= set(c)
    assert moved >= {'dt', 'bot_density', 'bot_linear_damping', 'bot_angular_damping', 'damping_model', 'obj_density', 'obj_friction',
                     'wall_friction', 'obj_linear_damping', 'obj_angular_damping'}
    dts = [c['dt'] for _, c, _ in GS.BOT_CONSTANTS if 'dt' in c]
    dens = [c['bot_density'] for _, c, _ in GS.BOT_CONSTANTS if 'bot_density' in c]
    assert min(dts) < 0.1 < max(dts) and min(dens) < 1.0 and max(dens) > 2.0
    clamped = [c for _, c, _ in GS.BOT_CONSTANTS if c.get('damping_model') == 1]
    assert clamped and all(1.0 - 0.1 * c['bot_linear_damping'] < 0.0 for c in clamped)


def run_containment(tmp_path, include=None):
    exe = compile_host(tmp_path, 'containment', CONTAINMENT_PROGRAM, include)
    cells = sorted({g.gw * g.gh for g in GS.GEOMETRY} | {2494})
    out = subprocess.run([exe], input='\n'.join(map(str, cells)).encode(), stdout=subprocess.PIPE, check=True).stdout.decode().strip().split('\n')
    return out[:-1], [int(x) for x in out[-1].split()]


def test_islmin_ends_inside_the_image_for_every_cell_count(tmp_path):
    """kb_step_kernel.h places islMin of the fixed-size kernel at ldsb::binE(...) whatever the plan says; below about 2070
    cells the NB words run past the bin table into the bytes the plan reserves behind the image."""
    violations, (bad, unplaced, over_bins, over_pairs, behind, fixed, behind_at_a_second_width) = run_containment(tmp_path)
    assert bad == 0 and unplaced == 0, violations
    assert over_bins > 0 and over_pairs > 0 and behind > 0           # all three placements occur in the sweep
    assert fixed >= GS.MAX_CELLS
    # islMin behind the image occurs at kb_create's width alone: that placement has no second width to test
    assert behind_at_a_second_width == 0
    assert all(g.N > GS.BOTS_PER_THREAD * (GS.WIDEST - 64) for g in GS.GEOMETRY if g.branch == 3)


def test_the_second_widths_take_the_placement_they_claim(tmp_path):
    rows = [next(g for g in GS.GEOMETRY if g.name == name) for name, _, _ in GS.SECOND_WIDTH]
    first = plans_of(tmp_path, rows)
    again = plans_of(tmp_path, rows, [width for _, width, _ in GS.SECOND_WIDTH])
    for (name, width, branch), (g, shape0, *_), (_, shape, variant, index, branch2, inside) in zip(GS.SECOND_WIDTH, first, again):
        assert g.sleep and not g.fn and shape0[5] != width and shape[5] == width and g.N <= GS.BOTS_PER_THREAD * width, name
        assert branch2 == branch and inside == 1 and variant[3] == 0, name
    assert {branch for _, _, branch in GS.SECOND_WIDTH} == {1, 2}


# ---- the oracle alone --------------------------------------------------------------------------------------------------
def run_on_oracle(s):
    """The launches of a scene on the oracle: (osim, per launch (phase, contacts (kilobot, wall, fixture), kilobots asleep,
    largest status word))"""
    osim = GS.oracle_sim(s)
    log = []
    for n, a, phase in s.launches:
        osim.set_actions(a)
        osim.step(n)
        log.append((phase, GS.oracle_contacts(osim), (osim.sleep_time < 0).sum(1).min() if s.kw['allow_sleep'] else 0, int(osim.status.max())))
    return osim, log


@pytest.mark.parametrize('g', GS.GEOMETRY, ids=GS.row_id)
def test_geometry_rows_are_not_vacuous_on_the_oracle(g):
    s = GS.scene(g)
    assert s.xy.shape == (GS.E, g.N, 2) and GS.E == 2 and not np.array_equal(s.xy[0], s.xy[1])
    assert np.abs(s.xy[..., 0]).max() <= g.W / 2 - 0.9 * g.r and np.abs(s.xy[..., 1]).max() <= g.H / 2 - 0.9 * g.r
    osim, log = run_on_oracle(s)
    print(g.name, log)
    assert all(status == 0 for _, _, _, status in log), log
    nb = max(c[0] for _, c, _, _ in log)
    nw = max(c[1] for _, c, _, _ in log)
    assert nb >= g.N // 4, 'kilobot contacts %d' % nb
    # a one-row grid: every kilobot on both walls where they are close enough for that, else (one wall at a time) half the
    # swarm on a wall besides the planted ones
    assert nw >= (2 * g.N if GS.on_two_walls(g) else g.N // 2 + 8 if g.gh == 1 else 8), 'wall contacts %d' % nw
    if g.family == 'objects':
        assert max(c[2] for _, c, _, _ in log) >= 2, log
    if g.sleep:
        rested = [asleep for phase, _, asleep, _ in log if phase == 'rest'][-1]
        woken = [asleep for phase, _, asleep, _ in log if phase == 'wake'][-1]
        assert rested >= 2 and woken < rested, 'asleep after the rest %d, after the wake launches %d' % (rested, woken)


_runs = {}


def constants_run(c):
    if c.name not in _runs:
        _runs[c.name] = run_on_oracle(GS.scene(c))
    return _runs[c.name]


@pytest.mark.parametrize('c', GS.CONSTANTS, ids=GS.row_id)
def test_constants_rows_act_on_the_oracle(c):
    osim, log = constants_run(c)
    assert all(status == 0 for _, _, _, status in log), log
    assert max(k[0] for _, k, _, _ in log) >= c.N // 4 and max(k[1] for _, k, _, _ in log) >= 8, log
    if c.kernel == 'objects':
        used = np.arange(osim.cap)[None, :] < osim.ws_cnt.astype(np.int64).sum(1)[:, None]
        assert ((osim.ws_key >= KEY_OBJ) & used).sum(1).min() >= 1, 'no kilobot-fixture contact in some env'
        assert (osim.ows_acc[:, GS.WALL_BOX, O.MAX_OBJECTS:, 0] >= 0).any(), 'the box on the wall has no wall manifold'
        assert (osim.ows_acc[:, :, O.MAX_OBJECTS:, 0] >= 0).any(-1).sum(1).min() >= 1
    if c.constant == 'default':
        return
    control, _ = constants_run(GS.control_of(c))
    if c.acts == 'bots':
        fields = [(f, getattr(osim, f), getattr(control, f)) for f in ('x', 'y', 'theta', 'ws_acc')]
    else:
        objs = list(c.acts)
        fields = [(f, getattr(osim, f)[:, objs], getattr(control, f)[:, objs]) for f in ('ox', 'oy', 'otheta', 'ows_acc')]
    differ = {f: int((word_bits(a) != word_bits(b)).sum()) for f, a, b in fields}
    print(c.name, differ)
    if c.acts == 'bots':
        # (equal masses cancel in a kilobot pair, so a density may show in the impulses alone.)  Not one stray word: as many
        # words as a quarter of the swarm
        assert sum(differ.values()) >= c.N // 4, differ
    else:
        assert differ['ox'] + differ['oy'] + differ['otheta'] >= 1, differ
