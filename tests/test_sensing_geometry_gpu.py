"""The sensing kernels and kb_render off the default arena: they walk the broadphase grid of the handle (inv_cell, gw, gh and
a reach in cells), which every other sensing suite holds at 58 x 43 cells of 0.875.  Here they run on the arenas and radii of
tests/geometry_scenes.py -- cells of 1.75 and 3.5, 103 x 78 cells, grids one and two cells thin, crowded cells -- against the
brute-force references of their own suites, which know nothing of a grid: kb_sense against the oracle's all-pairs count,
kb_sense_neighbors, kb_sense_histogram and kb_sense_reduce against the numpy restatements, the count fused into kb_step
against the oracle, kb_render against tests/render_ref.py with the arena taken from kb_get_outline.  The radii are half a
cell and one and a half cells of the row's own cell size, and the whole arena.  Everything is compared for equality."""
import numpy as np
import pytest
import torch

from tests import geometry_scenes as GS
from tests import scenes
from tests.gpu_common import assert_same, cpu, dev, geometry_pair as pair, ranges
from tests.sensing_checks import check_histogram, check_neighbors, check_reduce, check_render, messages

pytestmark = pytest.mark.gpu

ROWS = GS.SENSING_ROWS
RADII =('half-cell', 'cell-and-a-half', 'arena')
CASES = [(g, kind) for g in ROWS for kind in RADII]


def case_id(case):
    return '%s-%s' % (case[0].name, case[1])


def test_the_rows_cover_the_grids():
    assert {g.cell for g in ROWS} == {0.875, 1.75, 3.5}
    assert any(g.gh == 1 for g in ROWS) and any(g.gh == 2 for g in ROWS) and any(g.gw == 2 for g in ROWS)
    assert any(g.gw * g.gh > 8000 and g.N == 1024 for g in ROWS) and any(g.gw * g.gh < 2070 and g.N == 1024 for g in ROWS)
    assert any(g.r < 0.01 for g in ROWS) and any(g.family == 'objects' for g in ROWS)


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_sensing_entry_points_equal_brute_force(case):
    g, kind = case
    R = GS.sensing_radius(g, kind)
    s, osim, gsim = pair(g)
    got = cpu(gsim.sense(R)).view(np.uint32)
    want = osim.sense(R)
    assert np.array_equal(got, want), (g.name, R, int((got != want).sum()))
    if kind != 'half-cell':
        assert got.max() > 0
    if kind == 'arena':
        assert (got == g.N - 1).all()
    for k in (4, 16):
        check_neighbors(gsim, R, k, case_id(case))
    check_histogram(gsim, R, 4, 8, case_id(case))
    inr = ranges(gsim, R)
    values = messages(s.E, s.N, 2, 17)
    for op in ('sum', 'min'):
        check_reduce(gsim, inr, R, op, values, what=case_id(case))


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_fused_sensing_in_the_step(case):
    """kb_config.sense_radius: the counts of the last substep's sensing point equal the oracle's and kb_sense of the poses
    before that substep; the step itself stays bit exact."""
    g, kind = case
    R = GS.sensing_radius(g, kind)
    s, osim, gsim = pair(g, sense_radius=R)
    for k in range(2):
        a = scenes.random_actions(s.E, s.N, seed=60 + k)
        osim.set_actions(a)
        osim.step(3)
        gsim.step(2, actions=dev(a))
        before_last = cpu(gsim.sense(R)).view(np.uint32).copy()
        gsim.step(1)
        torch.cuda.synchronize()
        got = cpu(gsim.nbr_count).view(np.uint32)
        assert np.array_equal(got, osim.nbr_count), (g.name, kind, k)
        assert np.array_equal(got, before_last), (g.name, kind, k)
        assert_same(osim, gsim, '%s launch %d' % (case_id(case), k), s.fields)
    assert int(cpu(gsim.status).max()) == 0 and int(osim.status.max()) == 0


@pytest.mark.parametrize('name', ['2.0x0.06-40', '4.0x2.9-200', 'r0.04-200-sleep', 'objects-2.0x0.06'])
def test_render_off_the_default_arena(name):
    """64 x 48 pixels, all layers: a pixel is 2.3 kilobot diameters high in the corridor and a kilobot is five pixels wide at
    r = 0.04 m; the restatement takes the arena from kb_get_outline."""
    g = next(g for g in GS.GEOMETRY if g.name == name)
    s, osim, gsim = pair(g)
    half_w, half_h = np.float32(0.5) * (np.float32(g.W) * np.float32(25.0)), np.float32(0.5) * (np.float32(g.H) * np.float32(25.0))
    assert tuple(gsim.outline().arena) == (-half_w, half_w, -half_h, half_h)
    w = check_render(gsim, 64, 48, what=name)
    assert (w != 255).any()                               # kilobots are in the picture
