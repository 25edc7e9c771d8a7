"""The scenes of the coverage tests, shared by tests/test_coverage_cpu.py (which checks on the restatement alone that each
scene holds what it is there for) and tests/test_coverage_gpu.py (device against restatement).  Every scene is (x, y, th,
select): float32 [E, N] in world units and radians as the state tensors hold them, select uint8 [E, N] or None."""
import numpy as np

from tests import scenes
from tests.scenes import world
from tests.sensing_common import wall_scene

f32 = np.float32
DENSE_GRIDS = [(16, 12), (64, 48), (128, 128)]      # of dense(): cells wider than the lattice, where most kilobots own nothing, and narrower
TIE_GRID = (50, 75)         # on the default arena of 50 x 37.5 world units: cw = 1, ch = 0.5 exactly


def ties():
    """E = 3, N = 7 for TIE_GRID, whose cell centres are (-24.5 + ix, -18.5 + 0.5 iy): the first four kilobots sit two
    units left, right, above and below the centre (-0.5, -0.5) -- equidistant from it, pairwise from its whole column and row
    and from the diagonals through it --, two more mirror each other in the row y = -0.5, the last is alone.  Env 1 holds the
    same points under reversed indices, so every tie goes to another kilobot; env 2 holds them in a third order, and its
    kilobots 1 and 3 share one point."""
    pts = np.array([[-2.5, -0.5], [1.5, -0.5], [-0.5, 1.5], [-0.5, -2.5], [10.5, 5.0], [10.5, -6.0], [-20.0, 10.25]])
    both = np.array(pts)
    both[6] = both[5]
    xy = np.stack([pts, pts[::-1], both[[3, 5, 0, 6, 2, 1, 4]]])
    th = np.random.RandomState(31).uniform(-np.pi, np.pi, size=(3, 7))
    return f32(xy[..., 0]), f32(xy[..., 1]), f32(th), None


# (tie centre, half distance, axis) of ring_ties(): two kilobots mirror each other in the centre along the axis, in broadphase
# cells (0.875 wide, from (-25, -18.75)) of DIFFERENT rings around the centre's own cell; the one in the outer ring comes first
RING_TIES = [((-10.5, -8.5), 0.5, 'x', +1), ((-15.5, 10.0), 1.25, 'y', +1), ((14.5, -11.5), 2.0, 'x', -1), ((0.5, 0.0), 1.5, 'x', -1)]
RING_TIE_BOTS = 128


def ring_ties():
    """E = 3, N = 128 for TIE_GRID, ties that the ring search settles (128 kilobots are worth four rings, the scan of ties()
    none that settles anything).  Kilobots 0..3 and 4..7 are the pairs of RING_TIES, every coordinate a multiple of 1/8: each
    pair is equidistant from its centre and from the whole row or column of centres through it, the outer-ring member has the
    lower index, so the search meets the owner LAST and must walk on after the ring that holds the other; pairs lie in rings
    0|1, 1|2, 2|3 and 1|2.  Kilobots 8.. are the points of a 13 x 11 lattice that are at least three units from every tie
    centre.  Env 1 holds the same points under reversed indices (the owner is met first); env 2 in a third order, and its
    kilobots 126 and 127 share the points of two pair members."""
    outer, inner = [], []
    for (cx, cy), d, axis, sign in RING_TIES:
        off = np.array([d, 0.0]) if axis == 'x' else np.array([0.0, d])
        outer.append(np.array([cx, cy]) + sign * off)
        inner.append(np.array([cx, cy]) - sign * off)
    gx, gy = np.meshgrid(-23.625 + 3.875 * np.arange(13), -17.375 + 3.375 * np.arange(11))
    lattice = np.stack([gx.ravel(), gy.ravel()], -1)
    clear = np.min([np.hypot(lattice[:, 0] - c[0], lattice[:, 1] - c[1]) for c, _, _, _ in RING_TIES], 0) >= 3.0
    pts = np.concatenate([np.array(outer), np.array(inner), lattice[clear][:RING_TIE_BOTS - 8]])
    assert pts.shape == (RING_TIE_BOTS, 2) and (pts * 8 == np.rint(pts * 8)).all()
    third = pts[np.random.RandomState(32).permutation(RING_TIE_BOTS)]
    third[126], third[127] = pts[0], pts[6]
    xy = np.stack([pts, pts[::-1], third])
    th = np.random.RandomState(33).uniform(-np.pi, np.pi, size=(3, RING_TIE_BOTS))
    return f32(xy[..., 0]), f32(xy[..., 1]), f32(th), None


FAR_CORNER_KW = dict(bot_radius=0.04)       # the broadphase grid of far_corner(): 15 x 11 cells of 3.5


def far_corner():
    """E = 2, N = 1024 for a handle with FAR_CORNER_KW: all kilobots inside ONE corner cell of a small broadphase grid (env 0
    the cell at (xmin, ymin), env 1 the one at (xmax, ymax)).  1024 kilobots are worth eleven rings, more than most centres are
    from their far corner: those centres find nothing until the ring that holds the far corner of the grid, and end there."""
    rng = np.random.RandomState(34)
    x = np.stack([rng.uniform(-24.9, -21.6, 1024), rng.uniform(24.1, 24.9, 1024)])
    y = np.stack([rng.uniform(-18.65, -15.35, 1024), rng.uniform(16.35, 18.65, 1024)])
    return f32(x), f32(y), f32(rng.uniform(-np.pi, np.pi, size=(2, 1024))), None


def one():
    """E = 2, N = 1: the one kilobot in a corner of the arena (env 0) and outside it beyond the opposite corner (env 1)."""
    return f32([[-24.0], [31.0]]), f32([[-18.0], [25.5]]), f32([[0.3], [-2.0]]), None


def walls():
    """sensing_common.wall_scene: E = 4, N = 96 in the corners and along the walls, some outside the arena."""
    return world(*wall_scene(random_headings=True)) + (None,)


def dense():
    """E = 2, N = 1024 on a jittered lattice of pitch 1.125 world units, for DENSE_GRIDS: long chains in the cell lists."""
    return world(*scenes.lattice_spawn(2, 1024, seed=3)) + (None,)


def select():
    """E = 3, N = 333, a wide Gaussian: env 0 selects a random half, env 1 one kilobot, env 2 none."""
    x, y, th = world(*scenes.gaussian_spawn(3, 333, sigma=0.3, seed=12))
    sel = np.zeros((3, 333), dtype=np.uint8)
    rng = np.random.RandomState(13)
    sel[0] = (rng.rand(333) < 0.5) * rng.randint(1, 256, 333)       # (any non-zero byte selects)
    sel[1, 217] = 128
    return x, y, th, sel
