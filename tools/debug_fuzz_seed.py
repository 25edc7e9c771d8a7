"""Debug helper: one scene of tests/test_parity_fuzz_gpu.py (SEED=...), started and stepped like the test; prints every field
that differs after each launch.  SINGLE=1 splits every launch into single substeps and compares after each one, WS=1 compares
the packed warm-start list as well.  KB_HIP_LIB selects an experiment build."""
import os, sys
import numpy as np, torch
sys.path.insert(0, '.')
from tests import fuzz_scenes as FS
from tests.gpu_common import assert_ws_same, cpu, dev, make_pair

seed = int(os.environ.get('SEED', '0'))


def loud(osim, gsim, what='', fields=()):
    torch.cuda.synchronize()
    bad = False
    for f in tuple(fields) + ('ws_cnt',):
        a, b = getattr(osim, f), cpu(getattr(gsim, f))
        b = b.reshape(a.shape)
        if not np.array_equal(a, b, equal_nan=False):
            idx = np.argwhere(~(a == b))
            print(what, f, 'differs at', idx[:8].tolist(), 'oracle', a[tuple(idx[0])], 'gpu', b[tuple(idx[0])])
            bad = True
    if bad:
        print('oracle status', osim.status, 'gpu status', cpu(gsim.status))
        np.set_printoptions(precision=5, suppress=True, linewidth=200)
        for f in ('x', 'y', 'ox', 'oy', 'otheta', 'ovx', 'ovy', 'ow'):
            if getattr(osim, f, None) is not None and getattr(gsim, f, None) is not None:
                print(f, 'oracle', np.asarray(getattr(osim, f)).ravel()[:16]); print(f, 'gpu   ', cpu(getattr(gsim, f)).ravel()[:16])
        raise SystemExit(1)
    if os.environ.get('WS'):
        assert_ws_same(osim, gsim, what)

s = FS.scene(seed)
osim, gsim = make_pair(s.E, s.N, s.mode, s.light, xy=s.xy, th=s.th, **s.kw)
written = FS.start(s, osim)
if s.nobj:
    gsim.set_objects_m(s.objs, s.oth)
for name in written:
    getattr(gsim, name).copy_(dev(getattr(osim, name)).reshape(getattr(gsim, name).shape))
substeps = 0
for k, (n_sub, a, la) in enumerate(s.launches):
    if a is not None:
        osim.set_actions(a)
    ga, gla = None if a is None else dev(a), None if la is None else dev(la)
    for n in [1] * n_sub if os.environ.get('SINGLE') else [n_sub]:
        osim.step(n, light_action=la)
        gsim.step(n, actions=ga, light_action=gla)
        substeps += n
        torch.cuda.synchronize()
        if ((osim.status | cpu(gsim.status)) & ~2).any():
            # capacity or a staging limit: what the flagged env computes is unspecified, the test ends the scene here
            print('%s launch %d: status oracle %s gpu %s, the scene ends' % (s.what, k, osim.status, cpu(gsim.status)))
            raise SystemExit(0)
        loud(osim, gsim, '%s launch %d substep %d' % (s.what, k, substeps), s.fields)
print('seed', seed, 'ok')
