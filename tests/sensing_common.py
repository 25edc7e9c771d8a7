"""What the tests of every sensing kernel share and that needs neither torch nor a device to import: the scenes and the
sweep of the GPU tests, the sim they run on, and the reader of the code object's metadata of the CPU tests.  What touches
the device is in tests/gpu_common.py, the comparers against the restatements in tests/sensing_checks.py."""
import os
import re

import numpy as np

from gym_kilobots_amd import build as kb_build
from tests import hops_ref
from tests import scenes

# (E, N, R): cfg2 / cfg3 slices, odd sizes, N = 1; R from one cell to the whole arena (test_sense_equals_brute_force_oracle).
# (2, 7, 4.0): 25 R / 0.875 > 58 + 43 cells, the smallest shape on which the entry points clamp the reach to the whole grid
SWEEP = [(8, 64, 0.07), (8, 64, 0.3), (4, 1024, 0.05), (4, 1024, 0.1), (3, 333, 0.034), (2, 7, 0.5), (5, 1, 0.1), (2, 7, 4.0)]


def make_sim(E, N, xy=None, th=None, **kw):
    from gym_kilobots_amd.sim import KilobotSim
    kw.setdefault('allow_sleep', 0)
    g = KilobotSim(E, N, **kw)
    if xy is not None:
        g.set_poses_m(xy, th)
    return g


def sweep_scene(E, N):
    if N == 1024:
        return scenes.lattice_spawn(E, N, seed=3)
    return scenes.gaussian_spawn(E, N, sigma=0.2, seed=4)


def wall_scene(random_headings=False):
    """The scene of test_sense_at_walls_and_corners: kilobots in the corners and along the walls, some outside the arena
    (their cell indices clamp).  random_headings: drawn after the positions, from the same generator; otherwise zero."""
    N = 96
    rng = np.random.RandomState(9)
    xy = np.zeros((4, N, 2))
    corners = np.array([[-1.0, -0.75], [1.0, -0.75], [1.0, 0.75], [-1.0, 0.75]])
    for e in range(4):
        xy[e, :24] = corners[e] + rng.uniform(-0.03, 0.08, size=(24, 2)) * -np.sign(corners[e])
        xy[e, 24:48] = np.stack([rng.uniform(-1, 1, 24), np.full(24, 0.75 - 0.0165) + rng.uniform(-0.01, 0.03, 24)], -1)
        xy[e, 48:72] = np.stack([np.full(24, -1.0 + 0.0165) + rng.uniform(-0.03, 0.01, 24), rng.uniform(-0.75, 0.75, 24)], -1)
        xy[e, 72:] = rng.uniform(-0.2, 0.2, size=(24, 2))
    return xy, rng.uniform(-np.pi, np.pi, size=(4, N)) if random_headings else np.zeros((4, N))


def chain_scene():
    """The serpentine chain, its indices permuted, in two envs; returns (xy [2, 1024, 2], position of every index in the chain)."""
    pts = hops_ref.serpentine()
    perm = np.random.RandomState(5).permutation(1024)      # index i sits at chain position perm[i]
    return np.stack([pts[perm], pts[perm]]), perm


def world_xy(xy):
    return tuple((xy[:, k] * 25.0).astype(np.float32) for k in (0, 1))


def cloud():
    return world_xy(scenes.gaussian_spawn(1, 333, sigma=0.2, seed=4)[0][0])


def f32(v):
    return np.asarray(v, dtype=np.float32)


def kernel_metadata(name_substring):
    """[(kernel name, {key: value})] of the kernels of the kb_abi unit whose name contains name_substring, with the private
    segment size and the spill counts, from the metadata of the code object that was linked (the assembly build() keeps next
    to the object)."""
    asm = os.path.join(os.path.dirname(kb_build.LIB), '_obj', 'rel', 'kb_abi-hip-amdgcn-amd-amdhsa-gfx950.s')
    if not os.path.exists(asm):
        kb_build.build(force=True)
    found = []
    for doc in re.split(r'\n  - \.agpr_count:', open(asm).read())[1:]:
        name = re.search(r'\.name:\s+(\S*' + re.escape(name_substring) + r'\S*)', doc)
        if not name:
            continue
        fields = {}
        for key in ('.private_segment_fixed_size', '.sgpr_spill_count', '.vgpr_spill_count'):
            m = re.search(re.escape(key) + r':\s+(\d+)', doc)
            assert m, (name.group(1), key)
            fields[key] = int(m.group(1))
        found.append((name.group(1), fields))
    return found
