"""kb_sense_assign between guard bands (tests/guarded.py): the bound buffers of the sim, the points, both selections and all
five outputs lie in one arena with a canary band on both sides of each, at sizes where N and K are odd.  With every non-empty
subset of the outputs the call writes what a plain sim returns, no canary byte changes, no bound buffer of the handle changes
and an output that was not asked for is not touched."""
import itertools

import numpy as np
import pytest
import torch

from tests import guarded as GD
from tests import scenes
from tests.sensing_common import make_sim

pytestmark = pytest.mark.gpu

PARTS = ('index', 'rel', 'owner', 'dist', 'stats')
SUBSETS = [s for k in range(1, 6) for s in itertools.combinations(PARTS, k)]
CUTOFF = 0.4


@pytest.mark.parametrize('N,K', [(7, 5), (333, 129)])
def test_outputs_between_bands(N, K):
    E = 3
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.25, seed=45)
    rng = np.random.RandomState(46)
    pts = torch.from_numpy(rng.uniform([-1.0, -0.75], [1.0, 0.75], size=(E, K, 2)).astype(np.float32)).cuda()
    bsel = torch.from_numpy((rng.rand(E, N) < 0.7).astype(np.uint8)).cuda()
    ssel = torch.from_numpy((rng.rand(E, K) < 0.7).astype(np.uint8)).cuda()
    bsel[0, 0] = ssel[0, 0] = 1     # (env 0 has a pair at every size ...
    pts[0, 0] = 0.0                 # ... kilobot 0 and slot 0 are within the cutoff of each other)
    bsel[1] = 0                     # an env with an empty side writes its constants, and nothing else
    P = make_sim(E, N, xy, th)
    P.x[0, 0] = P.y[0, 0] = 0.0
    G, arena = GD.guarded_sim(lambda: make_sim(E, N, xy, th), extra=8 << 20)
    for name in GD.bound_fields(P):
        if name != 'scratch':
            getattr(G, name).copy_(getattr(P, name))
    gpts = arena.take(pts.shape, pts.dtype, 8 * K, 'points')
    gbsel = arena.take(bsel.shape, bsel.dtype, N, 'bot_select')
    gssel = arena.take(ssel.shape, ssel.dtype, K, 'slot_select')
    gpts.copy_(pts)
    gbsel.copy_(bsel)
    gssel.copy_(ssel)
    fresh = P.targets(pts, 0.03, bot_select=bsel, slot_select=ssel, match='greedy', cutoff_m=CUTOFF)
    assert int(fresh.index[0].max()) >= 0 and int(fresh.index[1].max()) == -1 and int(fresh.owner[1].max()) == -1 and float(fresh.stats[0, 3]) >= 1.0
    out = {n: arena.take(t.shape, t.dtype, t.numel() * t.element_size() // E, n) for n, t in zip(PARTS, fresh)}
    before = {name: GD.bits(getattr(G, name)).clone() for name in GD.bound_fields(G)}
    for subset in SUBSETS:
        for t in out.values():
            t.view(torch.uint8).fill_(0x5A)
        got = G.targets(gpts, 0.03, bot_select=gbsel, slot_select=gssel, match='greedy', cutoff_m=CUTOFF, out=tuple(out[n] for n in subset),
                        **{n: n in subset for n in PARTS})
        torch.cuda.synchronize()
        what = 'N = %d, K = %d, outputs %s' % (N, K, '+'.join(subset))
        arena.check(what)
        for n in PARTS:
            if n in subset:
                assert getattr(got, n).data_ptr() == out[n].data_ptr()
                assert torch.equal(GD.bits(out[n]), GD.bits(getattr(fresh, n))), '%s: %s differs' % (what, n)
            else:       # an output that was not asked for is not touched
                assert getattr(got, n) is None and bool((out[n].view(torch.uint8) == 0x5A).all()), '%s: %s was written' % (what, n)
        assert torch.equal(gpts, pts) and torch.equal(gbsel, bsel) and torch.equal(gssel, ssel)
        for name, kept in before.items():
            assert torch.equal(kept, GD.bits(getattr(G, name))), '%s: bound buffer %s changed' % (what, name)
    GD.assert_fields_equal(P, G, 'assign')
