"""The contact search and the island walks on the device against the oracle, on the scenes of
tests/contact_search_scenes.py (tests/test_contact_search_cpu.py shows on the oracle that they have owners with 3 .. 7
owned contacts and the long islands).  Per scene and sleep setting: plant, run 1 .. 3 single-substep launches, and compare
poses, commands, the packed warm-start list (ws_key, ws_acc, ws_cnt) and the status bit for bit after every launch; then
plant again with the next seed.  The scenes run a one-wave generic kernel (40 and 64 kilobots), a generic kernel of
several waves (200) and the fixed-size kernel (1024)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import contact_search_scenes as CS
from tests import solver_regimes as SR
from tests.gpu_common import make_pair, assert_same, assert_ws_same, cpu, dev
from tests.host_common import variants  # noqa: F401

pytestmark = pytest.mark.gpu

WAVES = {40: (1, 1), 64: (1, 1), 200: (2, 8), 1024: (8, 8)}         # N -> waves per workgroup, from .. to


@pytest.mark.parametrize('allow_sleep', [0, 1], ids=['nosleep', 'sleep'])
@pytest.mark.parametrize('s', CS.SCENES, ids=CS.scene_id)
def test_contact_search_is_bit_exact(s, allow_sleep, variants):
    osim, gsim = make_pair(CS.E, s.N, allow_sleep=allow_sleep)
    drive, light, obj, fn, tier, poly, sense, sleep = variants[gsim.variant_index]
    assert (drive, light, obj, sleep) == (O.DRIVE_VELOCITY, O.LIGHT_NONE, 0, allow_sleep), variants[gsim.variant_index]
    assert fn == (1024 if s.N == 1024 else 0), 'the handle runs instantiation %s' % (variants[gsim.variant_index],)
    nw = gsim.block_threads // SR.LANES
    assert WAVES[s.N][0] <= nw <= WAVES[s.N][1], nw
    fields = ('x', 'y', 'theta', 'cmd_vx', 'cmd_vy', 'cmd_w', 'status') + (('sleep_time',) if allow_sleep else ())
    for seed in CS.SEEDS:
        xy, th, _ = CS.plant(s, seed)
        osim.set_poses_m(xy, th)
        gsim.set_poses_m(xy, th)
        for k in range(seed):
            a = CS.actions(s, seed, k)
            osim.set_actions(a)
            osim.step(1)
            gsim.step(1, actions=dev(a))
            what = '%s sleep %d seed %d substep %d' % (s.name, allow_sleep, seed, k)
            assert_same(osim, gsim, what, fields)
            assert_ws_same(osim, gsim, what)
            if k == 0:
                hist = np.bincount(cpu(gsim.ws_cnt).astype(np.int64).ravel(), minlength=8)
                if 'piles' in s.parts:
                    assert all(hist[c] >= CS.E * (8 - c) for c in CS.OWNER_COUNTS), (what, hist)
                if 'chain' in s.parts:
                    assert CS.islands(cpu(gsim.ws_key)[0].view(np.uint32), cpu(gsim.ws_cnt)[0])[:2] == [CS.CHAIN, CS.RING], what
        assert int(osim.status.max()) == 0 and int(cpu(gsim.status).max()) == 0, (osim.status, cpu(gsim.status))
