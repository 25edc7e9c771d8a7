"""kb_sense_targets off the default arena and constants.  kb_targets_kernel is a pure brute force: it reads x, y and theta of
the handle and nothing of its broadphase geometry -- no cell size, no grid, no arena --, so the rows of
tests/geometry_scenes.py cannot take it down another path.  One row is kept as a smoke check that the entry point serves a
handle of another shape: the largest grid (103 x 78 cells on 3.6 x 2.7 m) with 1024 kilobots, on its start poses, against the
brute force of tests/targets_ref.py.  Everything is compared for equality."""
import numpy as np
import pytest

from tests import geometry_scenes as GS
from tests.gpu_common import dev
from tests.sensing_checks import check_targets
from tests.sensing_common import make_sim

pytestmark = pytest.mark.gpu

ROW = [g for g in GS.GEOMETRY if g.name == '3.6x2.7-1024-sleep']


def test_targets_equal_brute_force_on_the_largest_grid():
    assert len(ROW) == 1 and (ROW[0].gw, ROW[0].gh, ROW[0].N) == (103, 78, 1024)
    g = ROW[0]
    s = GS.scene(g)
    sim = make_sim(s.E, s.N, s.xy, s.th, **s.kw)
    points = np.random.RandomState(80).uniform([-g.W / 2, -g.H / 2], [g.W / 2, g.H / 2], size=(129, 2)).astype(np.float32)
    w = check_targets(sim, dev(points), 0.05, what=g.name, alone=False)
    assert (w.index >= 0).all() and (w.owner >= 0).all() and np.isfinite(w.stats).all()
