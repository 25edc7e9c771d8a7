"""The continuous step against the walls on the device, on the scenes of tests/toi_scenes.py (tests/test_toi_filter_cpu.py
shows on the oracle what they hold and that the rule of the collection is exact): kilobots at rest on every wall and in the
corners, kilobots rammed into them head-on, at the shallowest angles that still give an event and along a diagonal, start
and end distances on and one fp32 step around both thresholds, a block asleep on a wall.

Per scene and sleep setting: twelve single-substep launches, each compared with the oracle as bit patterns -- x, y, theta, the
commands v and w, the sleep times where they are carried, the packed warm-start list and the status --, then one fused launch
of ten substeps.  Env-substeps without a candidate go round the processing loop and its barriers, the others take the loop.
In every case both kinds occur among the single launches and inside the fused launch, and env 1 has both inside the fused
launch (its late rammers land in substeps 13 ... 19): tests/test_toi_filter_cpu.py counts the candidates per env-substep and
asserts that.  The scenes of 1024 kilobots must run a fixed-size kernel, with and without the sleep
state, that of 200 a generic sorted-bin kernel of two waves, that of 16 a generic kernel."""
import numpy as np
import pytest

from tests import toi_scenes as TS
from tests.gpu_common import make_pair, assert_ws_same, cpu, dev
from tests.host_common import variants  # noqa: F401

pytestmark = pytest.mark.gpu


def assert_same_bits(osim, gsim, what, fields):
    for f in fields:
        a = getattr(osim, f)
        b = cpu(getattr(gsim, f)).reshape(a.shape)
        diff = a.view(np.uint32) != b.view(np.uint32)
        assert not diff.any(), '%s: %s differs in its bits at %s (%d of %d): oracle %r, device %r' % (
            what, f, np.argwhere(diff)[0], diff.sum(), diff.size, a[diff][0], b[diff][0])


@pytest.mark.parametrize('case', TS.cases(), ids=TS.case_id)
def test_continuous_step_is_bit_exact(case, variants):
    s, allow_sleep = case
    xy, th, acts, st, _ = TS.plant(s)
    E = xy.shape[0]
    osim, gsim = make_pair(E, s.N, allow_sleep=allow_sleep, bot_radius=s.radius)
    drive, light, obj, fn, tier, poly, sense, sleep = variants[gsim.variant_index]
    assert (obj, sleep) == (0, allow_sleep), variants[gsim.variant_index]
    assert fn == (1024 if s.N == 1024 else 0), 'the handle runs instantiation %s' % (variants[gsim.variant_index],)
    if s.N == 200:
        assert gsim.block_threads >= 128, 'a workgroup of at least two waves: %d threads' % gsim.block_threads
    fields = ('x', 'y', 'theta', 'v', 'w') + (('sleep_time',) if allow_sleep else ())
    osim.set_poses_m(xy, th)
    gsim.set_poses_m(xy, th)
    if allow_sleep:
        osim.sleep_time[...] = st
        gsim.sleep_time.copy_(dev(st))
    for k in range(TS.SINGLE_LAUNCHES + 1):
        n = 1 if k < TS.SINGLE_LAUNCHES else TS.FUSED_SUBSTEPS
        osim.set_actions(acts)
        osim.step(n)
        gsim.step(n, actions=dev(acts))
        what = '%s sleep %d launch %d (%d substeps)' % (s.name, allow_sleep, k, n)
        assert_same_bits(osim, gsim, what, fields)
        assert_ws_same(osim, gsim, what)
        assert np.array_equal(osim.status, cpu(gsim.status)[:E]), what
    assert int(osim.status.max()) == 0 and int(cpu(gsim.status).max()) == 0, (osim.status, cpu(gsim.status))
