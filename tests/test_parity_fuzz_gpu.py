"""Randomised parity sweep: many small random scenes (tests/fuzz_scenes.py: bot counts, drive laws, light models, object
shapes with random fixture-to-body maps, spawn densities, solver paths), each compared bit for bit with the oracle launch
by launch.

A scene ends early where the contact capacity overflows (status bit 0, oracle and device agree on it) or the device raises
a staging-limit flag (status bits 2 and 3) -- and a flag is held to the limits model (tests/limits_model.py), which the
oracle's trajectory is taken through substep by substep: the device may raise a bit in a launch only if the model finds that
limit exceeded in a substep of that launch or an earlier one (up to the first such substep the two trajectories are equal),
and where the model finds a limit exceeded the device must have raised the bit by the end of that launch."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import fuzz_scenes as FS
from tests import limits_model as LM
from tests.gpu_common import make_pair, assert_same, assert_ws_same, cpu, dev

pytestmark = pytest.mark.gpu

# how many scenes of a sweep leave at the capacity early-return (the overflow region must be measurable): counted
# per process, written behind the last scene to gpurun_out/fuzz_summary.txt (and printed with `pytest -s`)
COUNTS = {'scenes': 0, 'capacity_flag': 0, 'device_limit_flag': 0, 'slot_flag': 0}


@pytest.fixture(scope='module', autouse=True)
def _fuzz_summary():
    yield
    line = ('fuzz sweep: %(scenes)d scenes, %(capacity_flag)d left at the contact-capacity flag (status bit 0, oracle and device agree on it), '
            '%(device_limit_flag)d at a device-only staging limit (status bit 2), '
            '%(slot_flag)d compared to the end with the warm-start slot flag set (status bit 1)' % COUNTS)
    print(line)
    try:
        os.makedirs('gpurun_out', exist_ok=True)
        with open(os.path.join('gpurun_out', 'fuzz_summary.txt'), 'a') as f:
            f.write(line + '\n')
    except OSError:
        pass


@pytest.mark.parametrize('seed', FS.seeds())
def test_random_scene(seed):
    s = FS.scene(seed)
    osim, gsim = make_pair(s.E, s.N, s.mode, s.light, xy=s.xy, th=s.th, **s.kw)
    written = FS.start(s, osim)
    if s.nobj:
        gsim.set_objects_m(s.objs, s.oth)
    for name in written:
        getattr(gsim, name).copy_(dev(getattr(osim, name)).reshape(getattr(gsim, name).shape))
    shape = SimpleNamespace(threads=gsim.block_threads, staging=gsim.lds_staging_entries, capacity=gsim.contact_capacity)
    lim = LM.limits(s.N, shape.staging, shape.threads, plain=s.nobj == 0 and s.mode != O.DRIVE_MIXED)
    must, may = np.zeros(s.E, np.int32), np.zeros(s.E, np.int32)
    LIMIT_BITS = LM.BIT_STAGING | LM.BIT_CANDIDATES
    for k, (n_sub, a, la) in enumerate(s.launches):
        if a is not None:
            osim.set_actions(a)
        m1, m2 = FS.model_launch(osim, lim, shape, n_sub, la)
        must |= m1
        may |= m2
        gsim.step(n_sub, actions=None if a is None else dev(a), light_action=None if la is None else dev(la))
        torch.cuda.synchronize()
        so, sg = osim.status, cpu(gsim.status)
        if k == 0:
            COUNTS['scenes'] += 1
        if ((so | sg) & 1).any():
            COUNTS['capacity_flag'] += 1
            # contact capacity exceeded (absurdly dense spawn): which contacts are dropped is unspecified, only the flag is
            assert ((so & 1) == (sg & 1)).all(), 'capacity flag differs: %s vs %s' % (so, sg)
            return
        what = '%s launch %d: device status %s, the model asks for %s and allows %s' % (s.what, k, sg, must, may)
        assert ((sg & LIMIT_BITS & ~may) == 0).all(), 'a staging-limit flag that no limit accounts for -- ' + what
        assert ((must & ~sg) == 0).all(), 'a limit is exceeded and the device did not say so -- ' + what
        if (sg & LIMIT_BITS).any():
            COUNTS['device_limit_flag'] += 1
            # more kilobots on one fixture / in one rank group / ... than the device stages: what the flagged env computes is
            # unspecified, only the flag is
            return
        assert_same(osim, gsim, '%s step %d' % (s.what, k), s.fields)
        assert_ws_same(osim, gsim, 'seed %d step %d' % (seed, k))
    assert np.array_equal(osim.status & 3, cpu(gsim.status) & 3)     # (bits 2, 3 are limits of the device staging only: none was raised)
    if (osim.status & 2).any():
        COUNTS['slot_flag'] += 1
