"""The step kernels off the default arena and the default constants, bit for bit against the oracle: every row of the two
tables of tests/geometry_scenes.py (tests/test_geometry_cpu.py shows without a GPU that each row runs the grid, the bins,
the islMin placement and the kernel it claims, and that no scene is vacuous on the oracle).  After every launch the poses,
the commands, the status words, the sleep times, the object state and the packed warm-start list are compared; no scene
may leave through a flag -- the status words of both sides are 0 after every launch.  The handle must run what the
header plans for the row: instantiation, workgroup width, LDS bytes."""
import numpy as np
import pytest

from tests import geometry_scenes as GS
from tests.gpu_common import make_pair, assert_same, assert_ws_same, cpu, dev, put_device
from tests.host_common import plans_of, variants  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def planned(tmp_path_factory):
    """row name -> (plan fields, template arguments, index, islMin branch) at kb_create's width"""
    rows = GS.GEOMETRY + GS.CONSTANTS
    return {g.name: (shape, variant, index, branch) for g, shape, variant, index, branch, _ in plans_of(tmp_path_factory.mktemp('geometry'), rows)}


def run_row(g, plan, variants, threads=0):
    """One row on both sides, compared after every launch.  plan: what the header derives for the row at this width."""
    (_, cap, capL, nhead, hmask, width, lds_total, *_), variant, index, branch = plan
    s = GS.scene(g)
    osim, gsim = make_pair(s.E, s.N, s.mode, xy=s.xy, th=s.th, **s.kw)
    if threads:
        gsim.block_threads = threads
    exact = gsim._lib.kb_exact_division(gsim._h)
    print('ROW %s: variant %d %s, width %d, lds %d B, staged %d, capacity %d, %s bins (%d heads), islMin branch %d, exact_division %d'
          % (g.name, gsim.variant_index, variants[gsim.variant_index], gsim.block_threads, gsim.lds_bytes, gsim.lds_staging_entries,
             gsim.contact_capacity, 'hashed' if hmask else 'direct', nhead, branch if g.sleep else 0, exact))
    assert (gsim.variant_index, gsim.block_threads, gsim.lds_bytes, gsim.lds_staging_entries, gsim.contact_capacity) == \
        (index, width, lds_total, capL, cap), g.name
    assert tuple(variant) == variants[gsim.variant_index], g.name
    GS.apply_start(s, osim, GS.put_numpy)
    GS.apply_start(s, gsim, put_device)
    for k, (n, a, phase) in enumerate(s.launches):
        osim.set_actions(a)
        osim.step(n)
        gsim.step(n, actions=dev(a))
        what = '%s (exact_division %d, width %d) launch %d: %s of %d' % (g.name, exact, gsim.block_threads, k, phase, n)
        assert_same(osim, gsim, what, s.fields)
        assert_ws_same(osim, gsim, what)
        assert int(osim.status.max()) == 0 and int(cpu(gsim.status).max()) == 0, (what, osim.status, cpu(gsim.status))
    return osim, gsim


@pytest.mark.parametrize('g', GS.GEOMETRY, ids=GS.row_id)
def test_geometry_rows_are_bit_exact(g, planned, variants):
    osim, gsim = run_row(g, planned[g.name], variants)
    drive, light, obj, fn, tier, poly, sense, sleep = variants[gsim.variant_index]
    assert (fn, sleep) == (g.fn, g.sleep), variants[gsim.variant_index]
    if g.sleep:
        assert (cpu(gsim.sleep_time) > 0).any()           # the wake launches left kilobots awake and resting


@pytest.mark.parametrize('c', GS.CONSTANTS, ids=GS.row_id)
def test_constants_rows_are_bit_exact(c, planned, variants):
    run_row(c, planned[c.name], variants)


@pytest.mark.parametrize('name,second,branch', GS.SECOND_WIDTH)
def test_a_second_width_does_not_change_the_results(name, second, branch, planned, variants, tmp_path):
    g = next(g for g in GS.GEOMETRY if g.name == name)
    assert g.sleep and not g.fn and planned[g.name][0][5] != second
    (_, shape, variant, index, branch2, inside), = plans_of(tmp_path, [g], [second])
    assert shape[5] == second and inside == 1 and branch2 == branch
    print('ROW %s at width %d: islMin branch %d' % (g.name, second, branch2))
    _, first = run_row(g, planned[g.name], variants)
    _, again = run_row(g, (shape, variant, index, branch2), variants, threads=second)
    for f in ('x', 'y', 'theta', 'sleep_time', 'ws_cnt'):
        assert np.array_equal(cpu(getattr(first, f)), cpu(getattr(again, f))), f
