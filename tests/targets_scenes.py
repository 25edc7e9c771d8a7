"""The scenes of the targets tests, shared by tests/test_targets_cpu.py (which checks on the restatement alone that each scene
holds what it is there for) and tests/test_targets_gpu.py (device against restatement).  Every scene is a Scene(x, y, th,
points, tol, bsel, ssel): x, y, th float32 [E, N] in world units and radians as the state tensors hold them, points float32
[E, K, 2] or [K, 2] (shared) in METRES as kb_sense_targets takes them, tol the tolerance in metres, bsel uint8 [E, N] and ssel
uint8 [E, K] or None."""
import collections

import numpy as np

from tests import scenes
from tests.scenes import world
from tests.sensing_common import wall_scene

f32 = np.float32
Scene = collections.namedtuple('Scene', ('x', 'y', 'th', 'points', 'tol', 'bsel', 'ssel'))
ODD_SIZES = [(1, 1), (7, 5), (5, 7), (333, 129), (64, 1024), (1024, 3)]
SHARING_SIZES = [(64, 65), (65, 64), (128, 129), (129, 128), (300, 100)]      # of coarse(): around the sizes at which a side is shared out among the waves


def headings(seed, shape):
    return f32(np.random.RandomState(seed).uniform(-np.pi, np.pi, size=shape))


def ties():
    """E = 2, N = 7, K = 6; every coordinate in world units is a multiple of 0.125 (the slots are multiples of 0.125 m, which
    the one multiplication by 25 takes to multiples of 3.125 exactly), so equal distances are equal bit for bit.  Env 0: slot 2
    at (0, 0) lies between kilobots 1 at (1, 0) and 3 at (-1, 0); kilobot 0 at (9.375, 0) lies between slots 0 at (12.5, 0) and
    3 at (6.25, 0).  Env 1 holds the same kilobots and slots under reversed indices: there the lower index is the OTHER
    kilobot and the other slot, and it comes later in the order of env 0 -- a winner by position or by arrival is wrong in
    one of the two."""
    bots = np.array([[9.375, 0.0], [1.0, 0.0], [-20.0, 10.0], [-1.0, 0.0], [-10.0, -10.0], [16.125, 3.125], [-3.125, 6.5]])
    pts_w = np.array([[12.5, 0.0], [-18.75, 9.375], [0.0, 0.0], [6.25, 0.0], [15.625, 3.125], [-3.125, 6.25]])
    assert (bots * 8 == np.rint(bots * 8)).all() and (pts_w / 3.125 == np.rint(pts_w / 3.125)).all()
    xy = np.stack([bots, bots[::-1]])
    points = f32(np.stack([pts_w, pts_w[::-1]]) / 25.0)
    assert (points * f32(25.0) == np.stack([pts_w, pts_w[::-1]])).all()
    return Scene(f32(xy[..., 0]), f32(xy[..., 1]), headings(51, (2, 7)), points, 0.05, None, None)


def coincident():
    """E = 1, N = 3, K = 2: kilobot 1 sits exactly on slot 1, d2 = 0, and each is the other's nearest."""
    x, y = f32([[5.0, 3.125, -7.0]]), f32([[5.0, -6.25, 2.0]])
    return Scene(x, y, headings(52, (1, 3)), f32([[0.5, 0.5], [0.125, -0.25]]), 0.02, None, None)


def contested():
    """E = 1, N = 3, K = 2: kilobots 0 and 1 are both nearest to slot 0, which is nearest to kilobot 0: of the two exactly one
    is mutual.  Kilobot 2 and slot 1 hold each other."""
    x, y = f32([[0.5, -0.75, 10.0]]), f32([[0.0, 0.0, 10.0]])
    return Scene(x, y, headings(53, (1, 3)), f32([[0.0, 0.0], [0.5, 0.5]]), 0.02, None, None)


def odd(N, K):
    """E = 2, a Gaussian cloud of N kilobots and K slots drawn uniformly over the table, for the sizes of ODD_SIZES: one
    entry, fewer entries than lanes, sizes that fill no lane evenly, and one side at its limit."""
    x, y, th = world(*scenes.gaussian_spawn(2, N, sigma=0.25, seed=60 + N % 7))
    rng = np.random.RandomState(61 + K % 5)
    points = f32(rng.uniform([-1.0, -0.75], [1.0, 0.75], size=(2, K, 2)))
    return Scene(x, y, th, points, 0.03, None, None)


def parts_of(n_owners, n_other):
    """(parts, entries per part) into which kb_targets_side cuts the other side for a side of n_owners entries: four parts for
    at most 64 owners, two for at most 128, one otherwise; a part is a multiple of four entries."""
    parts = 4 if n_owners <= 64 else 2 if n_owners <= 128 else 1
    return parts, ((n_other + parts - 1) // parts + 3) & ~3


def coarse(N, K):
    """E = 2, kilobots and slots drawn from the 7 x 7 points of a lattice of pitch 0.125 m (3.125 world units, exact): most
    points hold several kilobots and several slots, so nearly every entry has its least d2 -- often zero -- with MANY entries of
    the other side, spread over all of its indices: whichever part of the other side a wave walks, the lower index must win.
    Env 1 holds env 0 under reversed indices."""
    rng = np.random.RandomState(67 + N + K)
    bots, pts = rng.randint(-3, 4, size=(N, 2)) * 3.125, rng.randint(-3, 4, size=(K, 2)) * 0.125
    xy, points = np.stack([bots, bots[::-1]]), f32(np.stack([pts, pts[::-1]]))
    return Scene(f32(xy[..., 0]), f32(xy[..., 1]), headings(68, (2, N)), points, 0.05, None, None)


def shared():
    """E = 3, N = 50, K = 40 with ONE set of points [K, 2] for all envs."""
    x, y, th = world(*scenes.gaussian_spawn(3, 50, sigma=0.3, seed=62))
    points = f32(np.random.RandomState(63).uniform([-1.0, -0.75], [1.0, 0.75], size=(40, 2)))
    return Scene(x, y, th, points, 0.03, None, None)


def outside():
    """sensing_common.wall_scene: E = 4, N = 96 in the corners and along the walls, some outside the arena; K = 24 slots on a
    ring of 1.3 m around the centre, most of them outside the arena of 2 x 1.5 m."""
    x, y, th = world(*wall_scene(random_headings=True))
    a = np.arange(24) * (2.0 * np.pi / 24)
    points = f32(np.stack([1.3 * np.cos(a), 1.3 * np.sin(a)], -1))
    return Scene(x, y, th, points, 0.05, None, None)


TOL = 0.0625        # of tolerance(): Tw = 1.5625 and T2 = 2.44140625 are exact


def tolerance():
    """E = 1, N = 3, K = 3 for tol = TOL (and for 0): kilobot 0 at the origin and slot 0 at (1.5625, 0) have d2 == T2 bit for
    bit, which is within tolerance; kilobot 1 at (23.4375, 2^-11) and slot 1 at (25, 0) have d2 = T2 + 2^-22, the next float,
    which is not; kilobot 2 sits on slot 2, the one pair within a tolerance of zero."""
    x, y = f32([[0.0, 23.4375, -12.5]]), f32([[0.0, 2.0 ** -11, -12.5]])
    return Scene(x, y, headings(54, (1, 3)), f32([[0.0625, 0.0], [1.0, 0.0], [-0.5, -0.5]]), TOL, None, None)


def cap():
    """E = 2, N = 5, K = 2, points per env.  Env 0: slot 1 lies 200 m = 5000 world units away, d2 = 2.5e7 and d2 * 65536 is
    above 2^40: its term of word 2 is the cap, word 0 has none.  Env 1: both slots are that far, every term of both sums is
    the cap."""
    x, y, th = world(*scenes.gaussian_spawn(2, 5, sigma=0.2, seed=64))
    points = f32([[[0.1, 0.1], [200.0, 0.0]], [[200.0, 0.0], [0.0, -200.0]]])
    return Scene(x, y, th, points, 0.05, None, None)


def masks():
    """E = 5, N = 300, K = 200: random 70 % selections on both sides, any non-zero byte selecting; env 2 selects no kilobot,
    env 3 no slot, env 4 neither."""
    x, y, th = world(*scenes.gaussian_spawn(5, 300, sigma=0.3, seed=65))
    rng = np.random.RandomState(66)
    points = f32(rng.uniform([-1.0, -0.75], [1.0, 0.75], size=(5, 200, 2)))
    bsel = ((rng.rand(5, 300) < 0.7) * rng.randint(1, 256, (5, 300))).astype(np.uint8)
    ssel = ((rng.rand(5, 200) < 0.7) * rng.randint(1, 256, (5, 200))).astype(np.uint8)
    bsel[2] = bsel[4] = 0
    ssel[3] = ssel[4] = 0
    return Scene(x, y, th, points, 0.03, bsel, ssel)


def full():
    """E = 2, N = K = 1024, the whole LDS image: the jittered lattice of pitch 0.045 m and as slots the plain lattice shifted
    by (0.02, 0.0125) m, shared by both envs; the shift is 0.0236 m long and the tolerance 0.025 m, which the jitter takes some
    kilobots out of."""
    x, y, th = world(*scenes.lattice_spawn(2, 1024, seed=3))
    plain, _ = scenes.lattice_spawn(1, 1024, seed=3, jitter=0.0)
    return Scene(x, y, th, f32(plain[0] + np.array([0.02, 0.0125])), 0.025, None, None)


SMALL = {'ties': ties, 'coincident': coincident, 'contested': contested, 'shared': shared, 'outside': outside, 'tolerance': tolerance,
         'cap': cap, 'masks': masks}
SMALL.update({'odd-%dx%d' % nk: (lambda nk=nk: odd(*nk)) for nk in ODD_SIZES})
SMALL.update({'coarse-%dx%d' % nk: (lambda nk=nk: coarse(*nk)) for nk in SHARING_SIZES})
SCENES = dict(SMALL, full=full)
