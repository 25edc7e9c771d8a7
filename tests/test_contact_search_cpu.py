"""The scenes of tests/contact_search_scenes.py without a GPU: on the oracle every scene has what it is there for -- in the
first substep after planting, owners with 3, 4, 5, 6 and 7 owned contacts (pile k gives exactly one owner of each count
0 .. k), the chain of 40 and the ring of 24 as one island each -- with status 0 in every substep of every launch sequence
that tests/test_contact_search_gpu.py runs.  Fails when a change of the scenes or of the broadphase grid lets a scene
silently lose its purpose; no scene is skipped."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import contact_search_scenes as CS


def first_substep(s, seed, allow_sleep=0):
    xy, th, ids = CS.plant(s, seed)
    osim = O.OracleSim(O.default_config(CS.E, s.N, allow_sleep=allow_sleep))
    osim.set_poses_m(xy, th)
    osim.set_actions(CS.actions(s, seed, 0))
    osim.step(1)
    return osim, xy, ids


def test_the_planted_structures_are_what_the_docstring_says():
    rng = np.random.RandomState(0)
    p = CS.piles(rng)
    at = 0
    for k in CS.PILE_KS:
        pile = p[at:at + k + 1]
        at += k + 1
        d = np.linalg.norm(pile[:, None] - pile[None], axis=-1)
        assert d.max() <= CS.PILE_SPREAD and d[~np.eye(k + 1, dtype=bool)].min() > 1e-5
        cells = np.floor((pile - [CS.XMIN, CS.YMIN]) / CS.CELL).astype(int)
        assert (cells == cells[0]).all(), 'pile %d straddles cells' % k
    assert at == CS.PILE_BOTS == 35
    c = CS.chain_and_ring(rng)
    row, ring = c[:CS.CHAIN], c[CS.CHAIN:]
    assert np.linalg.norm(np.diff(row, axis=0), axis=-1).max() < CS.DIAMETER
    assert np.linalg.norm(row[2:] - row[:-2], axis=-1).min() > CS.DIAMETER           # only neighbours touch
    assert np.linalg.norm(ring - np.roll(ring, 1, axis=0), axis=-1).max() < CS.DIAMETER
    assert np.linalg.norm(ring - np.roll(ring, 2, axis=0), axis=-1).min() > CS.DIAMETER
    assert len(set(map(tuple, np.floor((row - [CS.XMIN, CS.YMIN]) / CS.CELL).astype(int)))) >= 30       # many cells
    assert {s.N for s in CS.SCENES} == {40, 64, 200, 1024}
    assert all('piles' in s.parts or 'chain' in s.parts for s in CS.SCENES)


@pytest.mark.parametrize('seed', CS.SEEDS)
@pytest.mark.parametrize('s', CS.SCENES, ids=CS.scene_id)
def test_scene_has_its_owners_and_islands_on_the_oracle(s, seed):
    osim, xy, ids = first_substep(s, seed)
    assert int(osim.status.max()) == 0, osim.status
    for e in range(CS.E):
        cnt = osim.ws_cnt[e].astype(np.int64)
        hist = np.bincount(cnt, minlength=8)
        sizes = CS.islands(osim.ws_key[e], osim.ws_cnt[e])
        print('%s seed %d env %d: owned contacts 0 .. 7 %s, largest islands %s' % (s.name, seed, e, hist, sizes[:4]))
        assert len(hist) == 8, 'an owner with more than 7 contacts: %s' % hist
        at = 0
        if 'piles' in s.parts:
            for k in CS.PILE_KS:
                # one cell, everybody touches everybody: the kilobot in slot j of the cell owns the k - j behind it
                assert sorted(cnt[ids[e, at:at + k + 1]]) == list(range(k + 1)), (k, cnt[ids[e, at:at + k + 1]])
                at += k + 1
            assert all(hist[c] >= 8 - c for c in CS.OWNER_COUNTS), hist
            assert sizes[:3] == [8, 7, 6] or 'chain' in s.parts
        if 'chain' in s.parts:
            assert sizes[0] == CS.CHAIN >= 40 and sizes[1] == CS.RING, sizes[:4]
            assert cnt[ids[e, at:]].sum() == CS.CHAIN - 1 + CS.RING
        # the loose lattice touches nobody
        loose = np.setdiff1d(np.arange(s.N), ids[e])
        assert cnt[loose].sum() == 0, cnt[loose]


@pytest.mark.parametrize('allow_sleep', [0, 1], ids=['nosleep', 'sleep'])
@pytest.mark.parametrize('s', CS.SCENES, ids=CS.scene_id)
def test_every_launch_of_the_device_test_has_status_zero_on_the_oracle(s, allow_sleep):
    for seed in CS.SEEDS:
        osim, _, _ = first_substep(s, seed, allow_sleep)
        for k in range(1, seed):
            osim.set_actions(CS.actions(s, seed, k))
            osim.step(1)
        assert int(osim.status.max()) == 0, (s.name, seed, osim.status)
