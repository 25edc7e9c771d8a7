"""The scenes of the assign tests, shared by tests/test_assign_cpu.py (which checks on the restatement alone that each scene
holds what it is there for) and tests/test_assign_gpu.py (device against restatement).  Every scene is a Scene(x, y, th,
points, tol, cutoff, bsel, ssel): x, y, th float32 [E, N] in world units and radians as the state tensors hold them, points
float32 [E, K, 2] or [K, 2] (shared) in METRES as kb_sense_assign takes them, tol and cutoff in metres (cutoff None: no cutoff),
bsel uint8 [E, N] and ssel uint8 [E, K] or None."""
import collections

import numpy as np

from tests import scenes
from tests.scenes import world
from tests.targets_scenes import headings

f32 = np.float32
Scene = collections.namedtuple('Scene', ('x', 'y', 'th', 'points', 'tol', 'cutoff', 'bsel', 'ssel'))
# one entry; fewer entries than lanes with either side the shorter; a side one past and one short of a wave, and of the 256
# lanes that own the entries of a side
CLOUD_SIZES = [(1, 1), (7, 5), (5, 7), (65, 63), (257, 255)]


def cloud(N, K, E=2):
    """A Gaussian cloud of N kilobots against K slots drawn uniformly over the table, points per env: the kilobots in the
    middle contend for the same slots, those outside wait for what is left."""
    x, y, th = world(*scenes.gaussian_spawn(E, N, sigma=0.25, seed=80 + N % 7))
    points = f32(np.random.RandomState(81 + K % 5).uniform([-1.0, -0.75], [1.0, 0.75], size=(E, K, 2)))
    return Scene(x, y, th, points, 0.03, None, None, None)


def chain():
    """E = 1, N = K = 64: slots and kilobots alternate on the line y = 0 from x = -20 world units on, slot 0 first, and the gap
    after the i-th of the 128 points is 0.5 - 0.003 i: every gap is shorter than the one before.  Only the last pair is
    mutual at first; every other kilobot prefers the slot to its right, which prefers the kilobot to ITS right: one pair per
    round, min(N, K) = 64 rounds, the bound of the round loop."""
    pos = -20.0 + np.concatenate([[0.0], np.cumsum(0.5 - 0.003 * np.arange(127))])
    x = f32(pos[1::2])[None]
    points = np.zeros((64, 2), dtype=np.float32)
    points[:, 0] = f32(pos[0::2] / 25.0)
    return Scene(x, np.zeros_like(x), headings(82, (1, 64)), points, 0.01, None, None, None)


TIE_PITCH = 3.125       # world units: 0.125 m, so that slots in metres, their products with 25 and every difference are exact


def ties():
    """E = 2, N = K = 64: the 8 x 8 lattice of pitch 3.125 world units against the same lattice shifted by half a pitch both
    ways; every coordinate is exact, so equal distances are equal bit for bit: few distinct d2 among the 4096 pairs, and
    every choice is decided by the index.  Env 1 holds env 0 under reversed indices."""
    g = np.arange(8) - 4.0
    bots = np.stack(np.meshgrid(g, g, indexing='xy'), -1).reshape(64, 2) * TIE_PITCH
    pts_w = bots + 0.5 * TIE_PITCH
    points = f32(np.stack([pts_w, pts_w[::-1]]) / 25.0)
    assert (points * f32(25.0) == np.stack([pts_w, pts_w[::-1]])).all()
    xy = np.stack([bots, bots[::-1]])
    return Scene(f32(xy[..., 0]), f32(xy[..., 1]), headings(83, (2, 64)), points, 0.05, None, None, None)


def cutoff():
    """E = 2, N = 333, K = 129: a Gaussian cloud against uniform slots, 70 % of either side selected (any non-zero byte), and
    a cutoff of 0.25 m: slots far from the cloud stay free although kilobots are left over, and the other way round."""
    x, y, th = world(*scenes.gaussian_spawn(2, 333, sigma=0.2, seed=84))
    rng = np.random.RandomState(85)
    points = f32(rng.uniform([-1.0, -0.75], [1.0, 0.75], size=(2, 129, 2)))
    bsel = ((rng.rand(2, 333) < 0.7) * rng.randint(1, 256, (2, 333))).astype(np.uint8)
    ssel = ((rng.rand(2, 129) < 0.7) * rng.randint(1, 256, (2, 129))).astype(np.uint8)
    return Scene(x, y, th, points, 0.03, 0.25, bsel, ssel)


def full():
    """E = 1, N = K = 1024, the whole LDS image: a Gaussian cloud against the plain lattice of pitch 0.045 m."""
    x, y, th = world(*scenes.gaussian_spawn(1, 1024, sigma=0.25, seed=86))
    plain, _ = scenes.lattice_spawn(1, 1024, seed=3, jitter=0.0)
    return Scene(x, y, th, f32(plain[0]), 0.025, None, None, None)


def coincident():
    """E = 1, N = 4, K = 3: kilobots 1 and 2 at one position, slots 0 and 2 at one point, all four distances between them
    equal bit for bit.  The order (bits of d2, b, t) gives (1, 0) first, then (2, 2)."""
    x, y = f32([[10.0, 1.0, 1.0, -8.0]]), f32([[5.0, 2.0, 2.0, -3.0]])
    return Scene(x, y, headings(87, (1, 4)), f32([[0.125, 0.125], [0.5, 0.25], [0.125, 0.125]]), 0.02, None, None, None)


def on_a_slot():
    """E = 1, N = 3, K = 2 with cutoff_m = 0: kilobot 1 sits exactly on slot 1, d2 = 0 is not above C2 = 0 and the pair is
    matched; nothing else is admissible."""
    x, y = f32([[5.0, 3.125, -7.0]]), f32([[5.0, -6.25, 2.0]])
    return Scene(x, y, headings(88, (1, 3)), f32([[0.5, 0.5], [0.125, -0.25]]), 0.02, 0.0, None, None)


def empty_between():
    """E = 3, N = 40, K = 30: env 1 selects no kilobot, between two envs that select everything."""
    sc = cloud(40, 30, E=3)
    bsel, ssel = np.ones((3, 40), dtype=np.uint8), np.ones((3, 30), dtype=np.uint8)
    bsel[1] = 0
    return sc._replace(bsel=bsel, ssel=ssel)


def shared():
    """E = 3, N = 50, K = 40 with ONE set of points [K, 2] for all envs."""
    x, y, th = world(*scenes.gaussian_spawn(3, 50, sigma=0.3, seed=89))
    points = f32(np.random.RandomState(90).uniform([-1.0, -0.75], [1.0, 0.75], size=(40, 2)))
    return Scene(x, y, th, points, 0.03, None, None, None)


SMALL = {'chain': chain, 'ties': ties, 'cutoff': cutoff, 'coincident': coincident, 'on-a-slot': on_a_slot, 'empty-between': empty_between,
         'shared': shared}
SMALL.update({'cloud-%dx%d' % nk: (lambda nk=nk: cloud(*nk)) for nk in CLOUD_SIZES})
SCENES = dict(SMALL, full=full)
