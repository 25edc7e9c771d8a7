"""The label and flatten passes on the device against the oracle, on the scenes of tests/label_scenes.py
(tests/test_label_pass_cpu.py shows on the oracle that they have the long lists, full cells, owner changes, islands and wall
contacts they are there for, inside the LDS staging area).  Per scene and sleep setting: eight single-substep launches, each
compared bit for bit -- poses, the sleep times where they are carried, the packed warm-start list (ws_cnt, ws_key, ws_acc)
and the status --, then one fused launch of ten substeps.  The scenes of 1024 kilobots must run a fixed-size kernel (the
LDS read form of the union-find parents), the one of 200 a generic kernel (the volatile form, hashed bins)."""
import pytest

from tests import label_scenes as LS
from tests.gpu_common import make_pair, assert_same, assert_ws_same, cpu, dev
from tests.host_common import variants  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('allow_sleep', [0, 1], ids=['nosleep', 'sleep'])
@pytest.mark.parametrize('s', LS.SCENES, ids=LS.scene_id)
def test_label_pass_is_bit_exact(s, allow_sleep, variants):
    osim, gsim = make_pair(LS.E, s.N, allow_sleep=allow_sleep)
    drive, light, obj, fn, tier, poly, sense, sleep = variants[gsim.variant_index]
    assert (obj, sleep) == (0, allow_sleep), variants[gsim.variant_index]
    assert fn == (1024 if s.N == 1024 else 0), 'the handle runs instantiation %s' % (variants[gsim.variant_index],)
    fields = ('x', 'y', 'theta', 'status') + (('sleep_time',) if allow_sleep else ())
    xy, th = LS.plant(s)
    osim.set_poses_m(xy, th)
    gsim.set_poses_m(xy, th)
    for k in range(LS.SINGLE_SUBSTEPS + 1):
        n = 1 if k < LS.SINGLE_SUBSTEPS else LS.FUSED_SUBSTEPS
        a = LS.actions(s, k)
        osim.set_actions(a)
        osim.step(n)
        gsim.step(n, actions=dev(a))
        what = '%s sleep %d launch %d (%d substeps)' % (s.name, allow_sleep, k, n)
        assert_same(osim, gsim, what, fields)
        assert_ws_same(osim, gsim, what)
    assert int(osim.status.max()) == 0 and int(cpu(gsim.status).max()) == 0, (osim.status, cpu(gsim.status))
