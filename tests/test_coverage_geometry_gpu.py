"""kb_sense_coverage off the default broadphase grid: its search walks rings of the handle's own cells (inv_cell, gw, gh), which
tests/test_coverage_gpu.py holds at 58 x 43 cells of 0.875.  Here it runs on rows of tests/geometry_scenes.py -- cells of
0.875, 1.75 and 3.5, the one-row grid of 58 x 1 cells and the largest of 103 x 78 -- on their start poses, against the brute
force of tests/coverage_ref.py with the arena taken from kb_get_outline.  Everything is compared for equality."""
import numpy as np
import pytest

from tests import geometry_scenes as GS
from tests.sensing_checks import check_coverage
from tests.sensing_common import make_sim

pytestmark = pytest.mark.gpu

NAMES = ['2.0x0.034-40', '3.6x2.7-200-sleep', '3.6x2.7-1024-sleep', '4.0x2.9-200', 'r0.02-200', 'r0.04-200-sleep', 'r0.008-200']
ROWS = [g for g in GS.GEOMETRY if g.name in NAMES]


def test_the_rows_cover_the_grids():
    assert len(ROWS) == len(NAMES)
    assert {g.cell for g in ROWS} == {0.875, 1.75, 3.5}
    assert any((g.gw, g.gh) == (58, 1) for g in ROWS) and any((g.gw, g.gh) == (103, 78) and g.N == 1024 for g in ROWS)


@pytest.mark.parametrize('g', ROWS, ids=GS.row_id)
def test_coverage_equals_brute_force(g):
    s = GS.scene(g)
    sim = make_sim(s.E, s.N, s.xy, s.th, **s.kw)
    assert GS.grid(g.W, g.H, g.r) == (g.cell, g.gw, g.gh)
    half_w = np.float32(0.5) * (np.float32(g.W) * np.float32(25.0))
    assert sim.outline().arena[1] == half_w
    for gw, gh in ((64, 48), (7, 5)):
        w = check_coverage(sim, gw, gh, what=g.name, alone=False)
        assert (w.owner >= 0).all() and np.isfinite(w.stats).all()
