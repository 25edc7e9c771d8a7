"""The HIP path itself (through the C ABI) against the INDEPENDENT restatement of Box2D's step (tools/box2d_mini.py,
tests/golden/mini_solver.json): the same fixtures that pin the oracle on the CPU, replayed on the device with the same
float32 tolerances -- discrete solver, friction, block solver, polygon / circle / wall manifolds, polygons made by
b2PolygonShape::Set, compound bodies, and the continuous step of circles AND polygons (the mini-solver runs Box2D's general
b2TimeOfImpact on b2Distance there; the device its closed-form support-vertex distance).  The scenes come through
tests/mini_scenes.py, which builds the configuration from the object CLASSES the way the env does.

The polygon / compound / polygon-TOI scenes (those with a derived tolerance) are additionally held to the oracle bit for bit
at every step, with the comparison of the parity tests: a tolerance hit in the first test then says "the restatement of
Box2D is wrong" (oracle and kernel share it), not "the port is wrong"."""
import numpy as np
import pytest
import torch

from tests import mini_scenes as MS
from tests.mini_scenes import FIX

pytestmark = pytest.mark.gpu

_sim_for = MS.sim_for


@pytest.mark.parametrize('name', sorted(FIX))
def test_hip_path_follows_the_independent_solver(name):
    sc = FIX[name]
    g = _sim_for(sc)
    tol = sc['tol']
    for k, ref in enumerate(sc['trajectory']):
        for first, cmds in sc.get('commands', []):
            if first == k:
                g.set_actions(torch.tensor([cmds], dtype=torch.float32, device=g.x.device).contiguous())
        g.step(1)
        if sc.get('sleep'):          # the same substep falls asleep / wakes on the device as in the independent derivation
            st = g.sleep_time[0].double().cpu().numpy()
            want_s = np.array(ref['sleep'])
            assert np.array_equal(st < 0, want_s < 0) and np.abs(st - want_s).max() <= 1e-6, (name, k, 'sleep time', st, want_s)
            if sc['objects']:
                so = g.osleep[0].double().cpu().numpy()
                assert np.array_equal(so < 0, np.array(ref['osleep']) < 0), (name, k, 'object asleep', so)
        got = torch.stack([g.x[0], g.y[0], g.theta[0]], -1).double().cpu().numpy()
        want = np.array(ref['kilobots'])
        assert np.abs(got[:, :2] - want[:, :2]).max() <= tol, (name, k, 'kilobot position')
        assert np.abs(got[:, 2] - want[:, 2]).max() <= 10 * tol, (name, k, 'kilobot angle')
        if sc['objects']:
            o = torch.stack([g.ox[0], g.oy[0], g.otheta[0], g.ovx[0], g.ovy[0], g.ow[0]], -1).double().cpu().numpy()
            w = np.array(ref['objects'])
            assert np.abs(o[:, :2] - w[:, :2]).max() <= tol, (name, k, 'object position')
            assert np.abs(o[:, 2] - w[:, 2]).max() <= 10 * tol, (name, k, 'object angle')
            assert np.abs(o[:, 3:] - w[:, 3:]).max() <= 200 * tol, (name, k, 'object velocity')
    assert int(g.status.max().item()) == 0


@pytest.mark.parametrize('name', sorted(n for n in FIX if 'f32_f64_gap' in FIX[n]))
def test_hip_path_equals_the_oracle_bit_for_bit(name):
    """Poses, object poses and velocities, the manifold impulses with their feature ids (`ows_acc`), the kilobots' warm-start
    store and `status`, after every single-substep launch."""
    from tests.gpu_common import OBJ_FIELDS, assert_same, assert_ws_same
    sc = FIX[name]
    assert len(sc['kilobots']) <= 3 and len(sc['trajectory']) <= 80
    o, g = MS.oracle_for(sc), MS.sim_for(sc, debug_outputs=True)
    for k in range(len(sc['trajectory'])):
        o.step(1)
        g.step(1)
        assert_same(o, g, '%s step %d' % (name, k), OBJ_FIELDS + ('status',))
        assert_ws_same(o, g, '%s step %d' % (name, k))
    assert int(g.status.max().item()) == 0
