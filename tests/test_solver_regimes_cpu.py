"""The scenes of tests/solver_regimes.py without a GPU: on the oracle every scene visits exactly the solver regimes its
row claims, for at least the claimed number of substeps, with status 0 throughout -- classified with the band limits
(waves per workgroup, LDS staging entries, contact capacity) that the library derives for the scene's configuration, read
through the ABI (kb_create needs no GPU).  tests/test_solver_regimes_gpu.py runs the same scenes on the device; this file
fails when a change of plan_launch or of a scene lets one of them silently leave its regime."""
import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from oracle import oracle as O
from tests import solver_regimes as SR
from tests.host_common import lib  # noqa: F401

E = 2


def test_regime_follows_the_table():
    nw, capL, cap = 4, 832, 4096
    want = {0: 'R0', 128: 'R0', 129: None, 512: None, 513: 'R1', 832: 'R1', 833: 'R2', 2496: 'R2', 2497: 'R3', 4096: 'R3', 4097: None}
    assert {n: SR.regime(n, nw, capL, cap) for n in want} == want
    # the fixed-size kernel: 128 x 8 waves lie above its 688 staging entries -- no count is R1
    assert {SR.regime(n, 8, 688, 4160) for n in range(0, 4200)} == {'R0', None, 'R2', 'R3'}
    assert SR.regime(1025, 8, 688, 4160) == 'R2' and SR.regime(2064, 8, 688, 4160) == 'R2' and SR.regime(2065, 8, 688, 4160) == 'R3'
    assert SR.REG_CONTACTS == 128 and SR.GIANT_ISLAND >= SR.REG_CONTACTS


def test_the_scenes_cover_every_regime_of_every_kernel_size():
    by_size = {}
    for s in SR.SCENES:
        by_size.setdefault(s.N, set()).update(s.visits)
    assert by_size[200] == {'R0', 'R1', 'R2', 'R3'} and by_size[256] == {'R0', 'R1', 'R2', 'R3'}
    assert by_size[1024] == {'R0', 'R2', 'R3'}          # (no R1 by count at 1024 kilobots, see tests/solver_regimes.py)
    assert max(s.visits.get('R3', 0) for s in SR.SCENES if s.N == 1024) >= 3
    assert SR.REPLICA_SCENE.N == 1024 and SR.REPLICA_SCENE.visits == {'R3': SR.REPLICA_SCENE.substeps}


@pytest.mark.parametrize('allow_sleep', [0, 1], ids=['nosleep', 'sleep'])
@pytest.mark.parametrize('s', SR.SCENES, ids=SR.scene_id)
def test_scene_visits_its_regimes_on_the_oracle(lib, s, allow_sleep):
    band = SR.bands(lib, nat, s.N, s.capacity, allow_sleep)
    xy, th = SR.start(s, E)
    osim = O.OracleSim(O.default_config(E, s.N, **SR.config_kw(s, allow_sleep)))
    assert osim.cap == band[2]
    osim.set_poses_m(xy, th)
    seen, most = [], 0
    for k in range(s.substeps):
        osim.set_actions(SR.actions(E, s.N, k))
        osim.step(1)
        assert int(osim.status.max()) == 0, '%s substep %d: status %s' % (s.name, k, osim.status)
        seen.append(SR.classify(osim.ws_cnt, band))
        most = max(most, int(SR.counts(osim.ws_cnt).min()))
    osim.set_actions(SR.actions(E, s.N, s.substeps))
    osim.step(SR.FUSED_SUBSTEPS)                    # the fused launch that ends the device test
    assert int(osim.status.max()) == 0, '%s fused: status %s' % (s.name, osim.status)
    print(s.name, 'band (nw, capL, cap) = %s:' % (band,), ' '.join('/'.join(str(r) for r in row) for row in seen))
    SR.check_visits(s, seen)
    if set(s.visits) == {'R0'}:
        assert most >= SR.R0_MIN_CONTACTS, 'the register solver has next to nothing to do: at most %d contacts' % most


def test_sleeping_island_scene_on_the_oracle(lib):
    s = SR.SLEEP_SCENE
    band = SR.bands(lib, nat, s.N, s.capacity, 1)
    xy, th, sleep_time = SR.sleeping_island_start(E)
    osim = O.OracleSim(O.default_config(E, s.N, **SR.config_kw(s, 1)))
    osim.set_poses_m(xy, th)
    osim.sleep_time[...] = sleep_time
    seen = []
    for k in range(s.substeps + 1):
        osim.set_actions(SR.sleeping_island_actions(E, k))
        osim.step(1 if k < s.substeps else SR.FUSED_SUBSTEPS)
        assert int(osim.status.max()) == 0, (k, osim.status)
        # the 64 stay asleep with their 112 contacts in the list, nobody else sleeps
        assert (osim.sleep_time[:, :SR.SLEEPERS] < 0).all() and (osim.sleep_time[:, SR.SLEEPERS:] >= 0).all(), k
        assert (SR.sleeper_entries(osim.ws_cnt) == SR.SLEEPER_CONTACTS).all(), k
        if k < s.substeps:
            seen.append(SR.classify(osim.ws_cnt, band))
    SR.check_visits(s, seen)
    assert np.array_equal(osim.x[:, :SR.SLEEPERS], (xy[:, :SR.SLEEPERS, 0] * 25.0).astype(np.float32))      # asleep: not moved


def test_the_four_envs_of_the_replica_scene_stay_in_r3(lib):
    s, D = SR.REPLICA_SCENE, SR.REPLICA_ENVS
    band = SR.bands(lib, nat, s.N, s.capacity, 1)
    xy, th = SR.start(s, D)
    assert len({xy[e].tobytes() for e in range(D)}) == D          # four distinct envs
    osim = O.OracleSim(O.default_config(D, s.N, **SR.config_kw(s, 1)))
    osim.set_poses_m(xy, th)
    for k in range(s.substeps):
        osim.set_actions(SR.actions(D, s.N, k))
        osim.step(1, threads=D)
        assert int(osim.status.max()) == 0 and set(SR.classify(osim.ws_cnt, band)) == {'R3'}, (k, SR.counts(osim.ws_cnt), osim.status)
