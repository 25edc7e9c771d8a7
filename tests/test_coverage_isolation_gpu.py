"""kb_sense_coverage between guard bands (tests/guarded.py): the bound buffers of the sim and all four outputs lie in one arena
with a canary band on both sides of each, at sizes where gw * gh and N are odd.  With every non-empty subset of the outputs
the call writes what a plain sim returns, no canary byte changes and no bound buffer of the handle changes."""
import itertools

import numpy as np
import pytest
import torch

from tests import guarded as GD
from tests import scenes
from tests.sensing_common import make_sim

pytestmark = pytest.mark.gpu

PARTS = ('owner', 'dist', 'cells', 'stats')
SUBSETS = [s for k in range(1, 5) for s in itertools.combinations(PARTS, k)]


@pytest.mark.parametrize('gw,gh,N', [(7, 5, 7), (127, 95, 333)])
def test_outputs_between_bands(gw, gh, N):
    E = 3
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.25, seed=41)
    sel = torch.from_numpy((np.random.RandomState(42).rand(E, N) < 0.7).astype(np.uint8)).cuda()
    sel[1] = 0                  # an env without a candidate writes its constants, and nothing else
    P = make_sim(E, N, xy, th)
    G, arena = GD.guarded_sim(lambda: make_sim(E, N, xy, th), extra=8 << 20)
    for name in GD.bound_fields(P):
        if name != 'scratch':
            getattr(G, name).copy_(getattr(P, name))
    gsel = arena.take(sel.shape, sel.dtype, N, 'select')
    gsel.copy_(sel)
    fresh = P.coverage(gw, gh, select=sel)
    assert int(fresh.owner.max()) >= 0 and int(fresh.owner[1].max()) == -1
    shapes = {n: getattr(fresh, n) for n in PARTS}
    out = {n: arena.take(t.shape, t.dtype, t.numel() * t.element_size() // E, n) for n, t in shapes.items()}
    before = {name: GD.bits(getattr(G, name)).clone() for name in GD.bound_fields(G)}
    for subset in SUBSETS:
        for t in out.values():
            t.view(torch.uint8).fill_(0x5A)
        got = G.coverage(gw, gh, select=gsel, out=tuple(out[n] for n in subset), **{n: n in subset for n in PARTS})
        torch.cuda.synchronize()
        what = '%d x %d, N = %d, outputs %s' % (gw, gh, N, '+'.join(subset))
        arena.check(what)
        for n in PARTS:
            if n in subset:
                assert getattr(got, n).data_ptr() == out[n].data_ptr()
                assert torch.equal(GD.bits(out[n]), GD.bits(getattr(fresh, n))), '%s: %s differs' % (what, n)
            else:       # an output that was not asked for is not touched
                assert getattr(got, n) is None and bool((out[n].view(torch.uint8) == 0x5A).all()), '%s: %s was written' % (what, n)
        assert torch.equal(gsel, sel)
        for name, kept in before.items():
            assert torch.equal(kept, GD.bits(getattr(G, name))), '%s: bound buffer %s changed' % (what, name)
    GD.assert_fields_equal(P, G, 'coverage')
