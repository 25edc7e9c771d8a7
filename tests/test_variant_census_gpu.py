"""Every instantiation of kb_step_kernel, run once and compared bit for bit with the oracle: one case per row of
tests/golden/variant_census.txt (176 rows = the library's list, tests/test_variant_census_cpu.py).  Each case first checks
that the handle runs the instantiation the row is there for (kb_variant_index), then steps the scene of
tests/variant_census.py -- contacts, objects, lights, fused sensing and sleeping together, as far as the instantiation has
them -- through 45 single substeps and one fused launch of 10, comparing every field the configuration has after every
launch."""
import pytest
import torch

from tests import variant_census as VC
from tests.gpu_common import make_pair, assert_same, assert_ws_same, cpu, dev, put_device

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('row', VC.rows(), ids=VC.row_id)
def test_instantiation_equals_oracle(row):
    s = VC.scene(row)
    osim, gsim = make_pair(s.E, s.N, s.mode, s.light, xy=s.xy, th=s.th, **s.kw)
    if s.block_threads:
        gsim.block_threads = s.block_threads
    # first of all: the comparison is worth nothing on another kernel
    assert gsim.variant_index == s.index, 'the handle runs instantiation %d' % gsim.variant_index
    VC.apply_start(s, osim, VC.put_numpy)
    VC.apply_start(s, gsim, put_device)
    what = VC.row_id(row)
    done = 0
    for n, a, la in s.steps:
        VC.oracle_step(osim, (n, a, la))
        gsim.step(n, actions=None if a is None else dev(a), light_action=None if la is None else dev(la))
        done += n
        assert_same(osim, gsim, '%s, substep %d' % (what, done), s.fields)
        assert_ws_same(osim, gsim, '%s, substep %d' % (what, done))
    torch.cuda.synchronize()
    assert int(osim.status.max()) == 0 and int(cpu(gsim.status).max()) == 0
