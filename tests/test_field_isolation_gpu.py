"""kb_field_step between guard bands (tests/guarded.py): the bound buffers of the sim, the field, the amounts, the env mask
and the sense rows lie in one arena with a canary band on both sides of each, at sizes where gw * gh and N are odd.  With
and without a deposit, iterations, rows and a mask the call writes what a plain sim writes, no canary byte changes and no
bound buffer of the handle changes."""
import numpy as np
import pytest
import torch

from tests import guarded as GD
from tests import scenes
from tests.sensing_common import make_sim

pytestmark = pytest.mark.gpu

# (amount, iters, sense, mask)
JOBS = [(True, 2, True, False), (True, 0, True, True), (False, 3, False, False), (False, 0, True, False), (True, 1, False, True)]


@pytest.mark.parametrize('gw,gh,N,C', [(7, 5, 7, 1), (127, 95, 333, 3)])
def test_field_between_bands(gw, gh, N, C):
    E = 3
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.25, seed=41)
    rng = np.random.RandomState(43)
    P = make_sim(E, N, xy, th)
    G, arena = GD.guarded_sim(lambda: make_sim(E, N, xy, th), extra=8 << 20)
    for name in GD.bound_fields(P):
        if name != 'scratch':
            getattr(G, name).copy_(getattr(P, name))
    start = torch.from_numpy(rng.uniform(0.5, 1.5, (E, C, gh, gw)).astype(np.float32)).cuda()
    amount = torch.from_numpy(rng.uniform(-2.0, 2.0, (E, N, C)).astype(np.float32)).cuda()
    mask = torch.tensor([1, 0, 1], dtype=torch.uint8, device='cuda')
    gfield = arena.take(start.shape, start.dtype, C * gh * gw * 4, 'field')
    gamount = arena.take(amount.shape, amount.dtype, N * C * 4, 'amount')
    gmask = arena.take(mask.shape, mask.dtype, 1, 'env_mask')
    grows = arena.take((E, N, C, 4), torch.float32, N * C * 16, 'sense')
    gamount.copy_(amount)
    gmask.copy_(mask)
    keep, spread = (1.0, 0.9, 0.5)[:C], (0.25, 0.1, 0.0)[:C]
    before = {name: GD.bits(getattr(G, name)).clone() for name in GD.bound_fields(G)}
    for with_amount, iters, sense, masked in JOBS:
        what = '%d x %d, N = %d: amount %s, iters %d, sense %s, mask %s' % (gw, gh, N, with_amount, iters, sense, masked)
        field = start.clone()
        gfield.copy_(start)
        grows.view(torch.uint8).fill_(0x5A)
        rows = P.field_step(field, amount if with_amount else None, keep, spread, iters, mask if masked else None, sense)
        got = G.field_step(gfield, gamount if with_amount else None, keep, spread, iters, gmask if masked else None, sense, out=grows if sense else None)
        torch.cuda.synchronize()
        arena.check(what)
        assert torch.equal(GD.bits(gfield), GD.bits(field)), what
        assert (with_amount or iters > 0) == (not torch.equal(GD.bits(field), GD.bits(start))), what
        if sense:
            assert got.data_ptr() == grows.data_ptr()
            sel = [0, 2] if masked else [0, 1, 2]
            assert torch.equal(GD.bits(grows[sel]), GD.bits(rows[sel])), what
            assert not masked or bool((grows[1].view(torch.uint8) == 0x5A).all()), what
        else:
            assert got is None and bool((grows.view(torch.uint8) == 0x5A).all()), what
        assert torch.equal(gamount, amount) and torch.equal(gmask, mask), what
        for name, kept in before.items():
            assert torch.equal(kept, GD.bits(getattr(G, name))), '%s: bound buffer %s changed' % (what, name)
    GD.assert_fields_equal(P, G, 'field')
