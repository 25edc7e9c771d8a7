"""The scenes of the packed island placement (tests/test_placement_gpu.py, where the four families are described): touching
rectangles of kilobots 32.5 mm apart and single kilobots, at the smallest multi-wave shapes.  Shared with
tests/test_setup_fused_gpu.py."""
from types import SimpleNamespace

import numpy as np

from tests import scenes
from tests import setup_scenes as SS

E = 2
TOUCH = 0.0325                  # centre distance inside a rectangle (kilobot diameter 33 mm)
PITCH = 0.05                    # free space between motifs: more than a diameter

# rects: (columns, rows, how many); the rest of the N kilobots stand alone
# first: what the first launch must have -- (rule, one-slot waves in use, two-slot waves); later launches keep the rule and
# the band of contacts
_S = lambda name, N, nw, rects, band, first: SimpleNamespace(name=name, N=N, nw=nw, rects=rects, band=band, first=first)  # noqa: E731
SCENES = [
    _S('one-slot-200', 200, 2, [(2, 1, 60)], lambda nw: (32, 64 * (nw - 1)), ('packed', 1, 0)),
    _S('one-slot-256', 256, 4, [(3, 1, 40), (2, 1, 60)], lambda nw: (64, 64 * (nw - 1)), ('packed', 3, 0)),
    _S('mix-200', 200, 2, [(3, 1, 66), (2, 1, 1)], lambda nw: (64 * nw + 1, 128 * nw - 1), ('packed', 1, 1)),
    _S('mix-256', 256, 4, [(3, 3, 28)], lambda nw: (64 * nw + 1, 128 * nw - 1), ('packed', 2, 2)),
    _S('big-island-200', 200, 2, [(7, 7, 1), (2, 1, 75)], lambda nw: (65, 128 * nw), ('even', None, None)),
    _S('big-island-256', 256, 4, [(7, 7, 1), (2, 1, 100)], lambda nw: (65, 128 * nw), ('even', None, None)),
    _S('out-of-waves-200', 200, 2, [(4, 4, 10), (2, 1, 16)], lambda nw: (1, 128 * nw), ('even', None, None)),
]


def plant(s, seed):
    """(xy [E, N, 2] metres, theta [E, N]): the rectangles row by row on a loose grid, ids in no relation to places"""
    rng = np.random.RandomState(seed)
    xy = np.zeros((E, s.N, 2))
    for e in range(E):
        pts, x, y, tall = [], -0.93, -0.68, 0.0
        motifs = [(c, r) for c, r, n in s.rects for _ in range(n)]
        motifs += [(1, 1)] * (s.N - sum(c * r for c, r in motifs))
        for c, r in motifs:
            width = (c - 1) * TOUCH
            if x + width > 0.93:
                x, y, tall = -0.93, y + tall + PITCH, 0.0
            pts += [(x + i * TOUCH, y + j * TOUCH) for j in range(r) for i in range(c)]
            x += width + PITCH
            tall = max(tall, (r - 1) * TOUCH)
        assert y + tall < 0.70 and len(pts) == s.N, (s.name, y, len(pts))
        xy[e, rng.permutation(s.N)] = np.array(pts)
    th = rng.uniform(-np.pi, np.pi, size=(E, s.N))
    return xy, th


def actions(s, k):
    """U([0, 0.01] x [-pi/2, pi/2]) at 3 % of the speed: the rectangles press and drift without coming apart in 13 substeps"""
    a = scenes.random_actions(E, s.N, seed=400 + 10 * len(s.name) + k)
    a[..., 0] *= SS.SPEED
    return a
