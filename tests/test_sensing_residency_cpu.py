"""What tests/test_sensing_residency_gpu.py rests on, without a device: the distinct scene is what it is there for on the
oracle, the batch is larger than the machine, and the sensor table leaves out no sensing, field or render launch of
KilobotSim."""
import inspect
import re

import numpy as np
import pytest

from oracle import oracle as O
from tests import reduce_ref
from tests import residency_scenes as RS

# the public methods of KilobotSim that end in a kb_sense*, kb_field_step, kb_render or kb_light_sense launch: a new one
# needs a row in residency_scenes.SENSORS and a line here
SENSING_METHODS = ['clusters', 'contacts', 'coverage', 'edges', 'field_step', 'hops', 'light_sense', 'neighbor_histogram', 'neighbor_reduce',
                   'neighbors', 'object_points', 'occupancy_grid', 'paths', 'rays', 'render', 'sense', 'targets']
LAUNCH = re.compile(r"_call\(\s*'(kb_sense\w*|kb_field_step|kb_render|kb_light_sense)'")


@pytest.fixture(scope='module')
def run():
    return RS.oracle_run()


def degrees(o):
    return np.stack([reduce_ref.in_range(o.x[e], o.y[e], RS.RADIUS).sum(1) for e in range(RS.D)])


def contacts(o):
    """entries of the warm-start store per env: what kb_sense_contacts reads"""
    return o.ws_cnt.astype(np.int64).sum(1).tolist()


def test_the_scene_is_clean_and_has_contacts_in_every_env(run):
    assert run.status.tolist() == [0] * RS.D
    assert (run.ws_cnt.astype(np.int64).sum(1) > 0).all()
    assert contacts(run) == [438, 392, 431, 476, 426]
    assert (np.abs(run.x) < 25.0).all() and (np.abs(run.y) < 18.75).all(), 'a kilobot is outside the arena'


def test_the_light_does_not_change_the_scene(run):
    dark = RS.oracle_run(light=O.LIGHT_NONE)
    for f in ('x', 'y', 'theta', 'ws_cnt', 'ox', 'oy', 'otheta', 'status'):
        assert np.array_equal(getattr(run, f), getattr(dark, f)), f


def test_every_env_has_isolated_and_well_connected_kilobots(run):
    deg = degrees(run)
    assert deg.min(1).tolist() == [0] * RS.D
    assert all(19 <= m <= 22 for m in deg.max(1)), deg.max(1)
    isolated = (deg == 0).sum(1)
    assert all(13 <= k <= 21 for k in isolated), isolated


def test_the_five_envs_differ(run):
    deg = degrees(run)
    for e in range(RS.D):
        for f in range(e + 1, RS.D):
            assert not np.array_equal(deg[e], deg[f]), (e, f)
            assert not np.array_equal(run.x[e], run.x[f]), (e, f)
    assert len({tuple(p) for p in RS.LIGHTS_M.tolist()}) == RS.D
    v = RS.inputs()
    for name, a in v.items():
        if name != 'field_mask':
            assert len({a[e].tobytes() for e in range(RS.D)}) == RS.D, 'input %s is the same in two envs' % name
    assert v['field_mask'].tolist().count(0) == 1


def test_the_boxes_are_those_of_the_isolation_tests():
    from tests import test_state_isolation_gpu as SI
    assert RS.BOXES == SI.BOXES


@pytest.mark.parametrize('cus', [32, 64, 256, 304])
def test_the_batch_does_not_fit_the_machine(cus):
    for threads in (256, 512):
        W = RS.resident_workgroups(cus, threads)
        assert W == cus * 2048 // threads
        E = RS.batch_envs(RS.resident_workgroups(cus, 256))
        assert E % RS.D == 0 and E > W and E >= 2 * W and E - RS.D < 2 * RS.resident_workgroups(cus, 256)
    image = 4 * RS.PATHS_BIG_GRID[0] * RS.PATHS_BIG_GRID[1]
    W = RS.resident_by_lds(cus, image)
    E = RS.batch_envs(W)
    assert W == 2 * cus and E % RS.D == 0 and E > W and E - RS.D < 2 * W


def test_the_batch_on_256_cus():
    assert RS.resident_workgroups(256) == 2048 and RS.batch_envs(2048) == 4100
    assert RS.batch_envs(RS.resident_by_lds(256, 64 * 1024)) == 1025


def launching_methods():
    """The public methods of KilobotSim whose source launches a sensing kernel, themselves or through a private method."""
    from gym_kilobots_amd.sim import KilobotSim
    source = {name: inspect.getsource(fn) for name, fn in vars(KilobotSim).items() if inspect.isfunction(fn)}
    direct = {name for name, text in source.items() if LAUNCH.search(text)}
    private = {name for name in direct if name.startswith('_')}
    found = {name for name in direct if not name.startswith('_')}
    found |= {name for name, text in source.items() if not name.startswith('_') and any('self.%s(' % p in text for p in private)}
    return sorted(found)


def test_the_table_names_every_sensing_method():
    assert launching_methods() == sorted(SENSING_METHODS)
    assert sorted({row.method for row in RS.SENSORS}) == sorted(SENSING_METHODS)
    assert len({row.name for row in RS.SENSORS}) == len(RS.SENSORS)
    for row in RS.SENSORS + [RS.PATHS_BIG]:
        assert set(row.few) <= set(row.outputs) and callable(row.call)
