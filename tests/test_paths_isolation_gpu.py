"""kb_sense_paths between guard bands (tests/guarded.py) and over LDS that another kernel filled (kb_debug_lds): the bound
buffers of the sim, the source and blocked masks and all four outputs lie in one arena with a canary band on both sides of
each, at sizes where gw and N are odd.  With every non-empty subset of the outputs the call writes what a plain sim returns
over fresh LDS, no canary byte changes, an output that was not asked for is not touched and no bound buffer of the handle
changes."""
import itertools

import pytest
import torch

from gym_kilobots_amd import _native as nat
from tests import guarded as GD
from tests import objects_ref
from tests.paths_ref import random_masks
from tests.sensing_common import make_sim

pytestmark = pytest.mark.gpu

PARTS = ('dist', 'step', 'bots', 'stats')
SUBSETS = [s for k in range(1, 5) for s in itertools.combinations(PARTS, k)]
LDS_WORD = 1            # a small distance, a raised flag, a finite float
CLEAR = 0.0165


@pytest.mark.parametrize('N,gw,gh', [(7, 7, 5), (333, 33, 31)])
def test_outputs_between_bands(N, gw, gh):
    E = 3
    lib = nat.load()
    kw, centres = objects_ref.object_sets()['boxes']
    xy, th, objs, oth = objects_ref.spawn_over_objects(E, N, centres, seed=41)

    def make():
        g = make_sim(E, N, xy, th, **kw)
        g.set_objects_m(objs, oth)
        return g
    P = make()
    G, arena = GD.guarded_sim(make, extra=8 << 20)
    for name in GD.bound_fields(P):
        if name != 'scratch':
            getattr(G, name).copy_(getattr(P, name))
    source, blocked = (torch.from_numpy(m).cuda() for m in random_masks(E, gw, gh, seed=N, density=0.15))
    source[:, 0, :] = 1         # the bottom row lies clear of the boxes: sources that are free
    source[1] = 0               # an env without a source writes its constants, and nothing else
    gsrc, gblk = (arena.take(m.shape, m.dtype, gw * gh, n) for m, n in ((source, 'source'), (blocked, 'blocked')))
    gsrc.copy_(source)
    gblk.copy_(blocked)
    fresh = P.paths(gw, gh, source, blocked, clearance_m=CLEAR)._asdict()
    assert bool(torch.isfinite(fresh['dist'][0]).any()) and bool(torch.isinf(fresh['dist'][1]).all()) and not bool(fresh['stats'][1].any())
    out = {n: arena.take(t.shape, t.dtype, t.numel() * t.element_size() // E, n) for n, t in fresh.items()}
    before = {name: GD.bits(getattr(G, name)).clone() for name in GD.bound_fields(G)}
    for walls, gwalls in ((blocked, gblk), (None, None)):
        if walls is None:
            fresh = P.paths(gw, gh, source, None, clearance_m=CLEAR)._asdict()
        for subset in SUBSETS:
            for t in out.values():
                t.view(torch.uint8).fill_(0x5A)
            nat.check(lib.kb_debug_lds(0, LDS_WORD, None, G._stream()), 'kb_debug_lds')
            got = G.paths(gw, gh, gsrc, gwalls, clearance_m=CLEAR, out=tuple(out[n] for n in subset), **{n: n in subset for n in PARTS})
            torch.cuda.synchronize()
            what = 'N = %d, %d x %d, d_blocked %s, outputs %s' % (N, gw, gh, walls is not None, '+'.join(subset))
            arena.check(what)
            assert [getattr(got, n).data_ptr() for n in subset] == [out[n].data_ptr() for n in subset], what
            for n in PARTS:
                if n in subset:
                    assert torch.equal(out[n].view(torch.uint8), fresh[n].view(torch.uint8)), '%s: %s differs' % (what, n)
                else:       # an output that was not asked for is not touched
                    assert getattr(got, n) is None and bool((out[n].view(torch.uint8) == 0x5A).all()), '%s: %s was written' % (what, n)
            assert torch.equal(gsrc, source) and torch.equal(gblk, blocked)
            for name, kept in before.items():
                assert torch.equal(kept, GD.bits(getattr(G, name))), '%s: bound buffer %s changed' % (what, name)
    GD.assert_fields_equal(P, G, 'paths')
