"""kb_sense_clusters off the default broadphase grid: its stencil walks the handle's own cells (inv_cell, gw, gh), which
tests/test_clusters_gpu.py holds at 58 x 43 cells of 0.875.  Here it runs on rows of tests/geometry_scenes.py -- cells of
0.875, 1.75 and 3.5, the one-row grid of 58 x 1 cells and the largest of 103 x 78, 1024 kilobots, and 700 in the arena where the step
kernel hashes its bins above 512 kilobots and the sensing kernels keep plain heads -- on their start poses, against the brute force of tests/clusters_ref.py.
Everything is compared for equality."""
import numpy as np
import pytest

from tests import geometry_scenes as GS
from tests.gpu_common import ranges
from tests.sensing_checks import check_clusters
from tests.sensing_common import make_sim

pytestmark = pytest.mark.gpu

NAMES = ['2.0x0.034-40', '3.6x2.7-200-sleep', '3.6x2.7-700-sleep', '3.6x2.7-1024-sleep', '4.0x2.9-200', 'r0.02-200', 'r0.04-200-sleep', 'r0.008-200']
ROWS = [g for g in GS.GEOMETRY if g.name in NAMES]


def test_the_rows_cover_the_grids():
    assert len(ROWS) == len(NAMES)
    assert {g.cell for g in ROWS} == {0.875, 1.75, 3.5}
    assert any((g.gw, g.gh) == (58, 1) for g in ROWS) and any((g.gw, g.gh) == (103, 78) and g.N == 1024 for g in ROWS)
    assert any(g.N > 512 and g.hashed for g in ROWS)


@pytest.mark.parametrize('g', ROWS, ids=GS.row_id)
def test_clusters_equal_brute_force(g):
    s = GS.scene(g)
    sim = make_sim(s.E, s.N, s.xy, s.th, **s.kw)
    assert GS.grid(g.W, g.H, g.r) == (g.cell, g.gw, g.gh)
    select = np.random.RandomState(23).rand(s.E, s.N) < 0.75
    for R in (0.05, 0.12):
        inr = ranges(sim, R)
        for sel in (None, select):
            want = check_clusters(sim, inr, R, sel, what=g.name)
            assert (want[3][:, 0] >= 2).all() and (want[3][:, 1] >= 2).all()
