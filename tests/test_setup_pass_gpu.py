"""The register set-up of the solver (kb_regsolve_bins.inc: light load, depth pass, dealing, full load; the grouping pass of
kb_step_kernel.h in front of it) on the device against the oracle, on the scenes of tests/setup_scenes.py
(tests/test_setup_pass_cpu.py shows on the oracle that every scene has what it is there for and stays on the register path).
Per scene and sleep setting: twelve single-substep launches, each compared bit for bit -- poses, the sleep times where they are
carried, the packed warm-start list (ws_cnt, ws_key, ws_acc) and the status --, then one fused launch of ten substeps.  The
scenes of 1024 kilobots must run a fixed-size kernel, those of 200 a generic sorted-bin kernel of two waves."""
import pytest

from tests import setup_scenes as SS
from tests.gpu_common import make_pair, assert_same, assert_ws_same, cpu, dev
from tests.host_common import variants  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', SS.cases(), ids=SS.case_id)
def test_setup_pass_is_bit_exact(case, variants):
    s, allow_sleep = case
    E = len(s.envs)
    osim, gsim = make_pair(E, s.N, allow_sleep=allow_sleep)
    drive, light, obj, fn, tier, poly, sense, sleep = variants[gsim.variant_index]
    assert (obj, sleep) == (0, allow_sleep), variants[gsim.variant_index]
    assert fn == (1024 if s.N == 1024 else 0), 'the handle runs instantiation %s' % (variants[gsim.variant_index],)
    assert gsim.block_threads >= 128, 'workgroups of at least two waves: %d threads' % gsim.block_threads
    fields = ('x', 'y', 'theta', 'status') + (('sleep_time',) if allow_sleep else ())
    xy, th, st, ids = SS.plant(s)
    osim.set_poses_m(xy, th)
    gsim.set_poses_m(xy, th)
    if allow_sleep:
        osim.sleep_time[...] = st
        gsim.sleep_time.copy_(dev(st))
    else:
        st = st * 0
    for k in range(SS.SINGLE_LAUNCHES + 1):
        n = 1 if k < SS.SINGLE_LAUNCHES else SS.FUSED_SUBSTEPS
        a = SS.actions(s, k, st)
        osim.set_actions(a)
        osim.step(n)
        gsim.step(n, actions=dev(a))
        what = '%s sleep %d launch %d (%d substeps)' % (s.name, allow_sleep, k, n)
        assert_same(osim, gsim, what, fields)
        assert_ws_same(osim, gsim, what)
    assert int(osim.status.max()) == 0 and int(cpu(gsim.status).max()) == 0, (osim.status, cpu(gsim.status))
