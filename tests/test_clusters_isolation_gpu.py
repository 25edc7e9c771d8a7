"""kb_sense_clusters between guard bands (tests/guarded.py) and over LDS that another kernel filled (kb_debug_lds): the bound
buffers of the sim, the select and all four outputs lie in one arena with a canary band on both sides of each, at sizes
where N is odd.  With every subset of the optional outputs the call writes what a plain sim returns over fresh LDS, no canary
byte changes, an output that was not asked for is not touched and no bound buffer of the handle changes."""
import itertools

import numpy as np
import pytest
import torch

from gym_kilobots_amd import _native as nat
from tests import guarded as GD
from tests import scenes
from tests.sensing_common import make_sim

pytestmark = pytest.mark.gpu

PARTS = ('size', 'table', 'stats')
SUBSETS = [s for k in range(0, 4) for s in itertools.combinations(PARTS, k)]
LDS_WORD = 1            # a kilobot index, a small count, a finite float


@pytest.mark.parametrize('N,R', [(7, 0.2), (333, 0.05)])
def test_outputs_between_bands(N, R):
    E = 3
    lib = nat.load()
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.25, seed=41)
    sel = torch.from_numpy((np.random.RandomState(42).rand(E, N) < 0.7).astype(np.uint8)).cuda()
    sel[1] = 0                  # an env without a node writes its constants, and nothing else
    P = make_sim(E, N, xy, th)
    G, arena = GD.guarded_sim(lambda: make_sim(E, N, xy, th), extra=8 << 20)
    for name in GD.bound_fields(P):
        if name != 'scratch':
            getattr(G, name).copy_(getattr(P, name))
    gsel = arena.take(sel.shape, sel.dtype, N, 'select')
    gsel.copy_(sel)
    fresh = dict(zip(('label',) + PARTS, P.clusters(R, select=sel, size=True, table=True, stats=True)))
    assert int(fresh['size'].max()) >= 2 and int(fresh['label'][1].max()) == -1 and fresh['stats'][1].tolist() == [0, 0, -1, 0]
    out = {n: arena.take(t.shape, t.dtype, t.numel() * t.element_size() // E, n) for n, t in fresh.items()}
    before = {name: GD.bits(getattr(G, name)).clone() for name in GD.bound_fields(G)}
    for select, gselect in ((sel, gsel), (None, None)):
        if select is None:
            fresh = dict(zip(('label',) + PARTS, P.clusters(R, size=True, table=True, stats=True)))
        for subset in SUBSETS:
            for t in out.values():
                t.view(torch.uint8).fill_(0x5A)
            nat.check(lib.kb_debug_lds(0, LDS_WORD, None, G._stream()), 'kb_debug_lds')
            got = G.clusters(R, select=gselect, out=(out['label'],) + tuple(out[n] for n in subset), **{n: n in subset for n in PARTS})
            torch.cuda.synchronize()
            what = 'N = %d, select %s, outputs %s' % (N, select is not None, '+'.join(('label',) + subset))
            arena.check(what)
            got = (got,) if torch.is_tensor(got) else got
            assert [t.data_ptr() for t in got] == [out[n].data_ptr() for n in ('label',) + subset], what
            for n in ('label',) + PARTS:
                if n == 'label' or n in subset:
                    assert torch.equal(GD.bits(out[n]), GD.bits(fresh[n])), '%s: %s differs' % (what, n)
                else:       # an output that was not asked for is not touched
                    assert bool((out[n].view(torch.uint8) == 0x5A).all()), '%s: %s was written' % (what, n)
            assert torch.equal(gsel, sel)
            for name, kept in before.items():
                assert torch.equal(kept, GD.bits(getattr(G, name))), '%s: bound buffer %s changed' % (what, name)
    GD.assert_fields_equal(P, G, 'clusters')
