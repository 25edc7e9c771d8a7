"""The scenes of tests/label_scenes.py without a GPU: on the oracle every scene has, in the substeps that
tests/test_label_pass_gpu.py runs, what it is there for (owners with more than four list entries, cells of three and more
kilobots, pairs that change owner, long islands, kilobots that stay on a wall) and stays on the path the batched label
code runs on: never more contacts than the LDS staging area of its handle, status 0.  These are conditions on the scenes,
not measurements; they fail when a change of a scene, of the grid or of the launch plan lets a scene silently lose its
purpose."""
import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from oracle import oracle as O
from tests import label_scenes as LS
from tests import solver_regimes as SR
from tests.host_common import lib  # noqa: F401


def test_the_planted_structures_are_what_the_docstring_says():
    h = LS.hexagon(4)
    assert len(h) == 61 and len(LS.hexagon(3)) == 37
    d = np.linalg.norm(h[:, None] - h[None], axis=-1) * LS.SPACING
    near = (d < 0.033) & ~np.eye(61, dtype=bool)
    assert near.sum(axis=1).max() == 12 and near.sum(axis=1).min() >= 5       # first and second neighbours overlap
    f = LS.row_ring_walls()
    row, ring, wall = f[:LS.ROW], f[LS.ROW:LS.ROW + LS.RING], f[LS.ROW + LS.RING:]
    assert np.allclose(np.linalg.norm(np.diff(row, axis=0), axis=-1), LS.LINK)
    assert np.linalg.norm(ring - np.roll(ring, 1, axis=0), axis=-1).max() < 0.033
    assert np.linalg.norm(ring - np.roll(ring, 2, axis=0), axis=-1).min() > 0.033
    assert (np.abs(f[:, 0]) < 1.0 - 0.0149).all() and (np.abs(f[:, 1]) < 0.75 - 0.0149).all()
    assert len(wall) == LS.WALL_BOTS
    for s in LS.SCENES:
        xy, th = LS.plant(s)
        assert xy.shape == (LS.E, s.N, 2) and (np.abs(xy[..., 0]) < 0.99).all() and (np.abs(xy[..., 1]) < 0.74).all()
        assert len({tuple(np.round(p_, 5)) for p_ in xy[0]}) == s.N          # nobody planted twice
    assert [s.N for s in LS.SCENES] == [1024, 1024, 200]


@pytest.mark.parametrize('allow_sleep', [0, 1], ids=['nosleep', 'sleep'])
@pytest.mark.parametrize('s', LS.SCENES, ids=LS.scene_id)
def test_scene_has_on_the_oracle_what_it_is_there_for(lib, s, allow_sleep):
    nw, capL, cap = SR.bands(lib, nat, s.N, 0, allow_sleep)
    xy, th = LS.plant(s)
    osim = O.OracleSim(O.default_config(LS.E, s.N, allow_sleep=allow_sleep))
    assert osim.cap == cap
    osim.set_poses_m(xy, th)
    seen, before = [], None
    for k in range(LS.SINGLE_SUBSTEPS):
        osim.set_actions(LS.actions(s, k))
        osim.step(1)
        assert int(osim.status.max()) == 0, (s.name, k, osim.status)
        f = LS.substep_features(osim, before)
        before = [(fe['pairs'], fe['walls']) for fe in f]
        seen.append(f)
        print('%s sleep %d substep %d: ' % (s.name, allow_sleep, k) + ' | '.join(
            'contacts %d, owners > 4 entries %d (longest %d), fullest cell %d, largest island %d, owner changes %d, walls %d (kept %d)'
            % (fe['contacts'], fe['long_owners'], fe['longest'], fe['fullest_cell'], fe['island'], fe['owner_changes'], len(fe['walls']), fe['walls_kept'])
            for fe in f))
    osim.set_actions(LS.actions(s, LS.SINGLE_SUBSTEPS))
    osim.step(LS.FUSED_SUBSTEPS)
    assert int(osim.status.max()) == 0, (s.name, 'fused', osim.status)
    for e in range(LS.E):
        col = [f[e] for f in seen]
        # the LDS path: the staged contacts and, one substep on, the previous list fit the staging area
        assert all(fe['contacts'] <= capL for fe in col), (s.name, e, [fe['contacts'] for fe in col], capL)
        assert all(fe['contacts'] > 0 for fe in col)
        if 'long lists' in s.has:
            assert sum(fe['long_owners'] >= 1 for fe in col) >= LS.BATCHED_KEYS_SUBSTEPS, [fe['long_owners'] for fe in col]
        if 'full cells' in s.has:
            assert all(fe['fullest_cell'] >= 3 for fe in col), [fe['fullest_cell'] for fe in col]
        if 'owner changes' in s.has:
            assert sum(fe['owner_changes'] for fe in col) >= 1
        if 'islands' in s.has:
            assert col[0]['island'] >= LS.ISLAND, col[0]['island']
        if 'walls' in s.has:
            assert sum(fe['walls_kept'] >= 1 for fe in col) >= 3, [fe['walls_kept'] for fe in col]
    if s.chains:
        assert seen[0][0]['island'] >= LS.ROW


def test_the_fixed_size_scenes_select_the_fixed_size_kernels(tmp_path):
    from tests import variant_census as VC
    listed, selected = VC.host_census(tmp_path, [SR.plan_inputs(s.N, 0, sl) for s in LS.SCENES for sl in (0, 1)])
    at = 0
    for s in LS.SCENES:
        for sl in (0, 1):
            status, index = selected[at]
            at += 1
            drive, light, obj, fn, tier, poly, sense, sleep = listed[index]
            assert status == 0 and (obj, sleep) == (0, sl) and fn == (1024 if s.N == 1024 else 0), (s.name, listed[index])
