"""Every sensing, field and render kernel on more workgroups than the machine holds (tests/residency_scenes.py).

`small` has the D = 5 distinct envs, `big` the same five tiled to twice the workgroups that can be resident at once by the
hardware's bound of 32 waves per CU.  Per sensor: small equals the restatement of the kernel's definition on the state as it
is on the device, bit for bit; every replica of big equals small, every output, every env, bit for bit; a second launch
into the same tensors -- which starts on the first one's LDS -- gives the same bits; and the five envs' outputs differ, so
that a workgroup that picked up another env's leftovers could not pass.  Workgroups of several envs share a CU here, and
those of the later generations start on LDS that another env of the same kernel left behind: what a missing barrier between
waves or a word read before it is written needs in order to show.  Two negative controls change one kilobot of the LAST env
of big and require that the comparison reports that env and no other: it reaches the last generation.  No tolerances anywhere."""
import time

import numpy as np
import pytest
import torch

from gym_kilobots_amd import _native as nat
from oracle import oracle as O
from tests import assign_ref
from tests import edges_ref
from tests import field_ref
from tests import grid_ref
from tests import guarded as GD
from tests import hops_ref
from tests import objects_ref
from tests import paths_ref
from tests import rays_ref
from tests import reduce_ref
from tests import residency_scenes as RS
from tests import sensing_checks as SC
from tests.gpu_common import cpu, dev, object_state, ranges, state

pytestmark = pytest.mark.gpu

D = RS.D
OUTPUT_LIMIT = 256 << 20                                # bytes of the largest single output of a row
FRESH = {('edges', 'offsets'), ('edges', 'count')}      # outputs that edges() allocates itself on every call


# ---- the pair -------------------------------------------------------------------------------------------------------------
def cu_count():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def new_sim(E, n):
    """The distinct scene tiled to E envs after its six single-substep launches."""
    from gym_kilobots_amd.sim import KilobotSim
    reps = E // D
    assert reps * D == E
    xy, th, objs, a = RS.spawn(n)
    sim = KilobotSim(E, n, O.DRIVE_VELOCITY, O.LIGHT_CIRCULAR, debug_outputs=True, **RS.config_kw())
    sim.set_poses_m(np.tile(xy, (reps, 1, 1)), np.tile(th, (reps, 1)))
    sim.set_objects_m(np.tile(objs, (reps, 1, 1)))
    sim.light_x.copy_(dev(np.tile(RS.LIGHTS_M[:, 0], reps)))
    sim.light_y.copy_(dev(np.tile(RS.LIGHTS_M[:, 1], reps)))
    a = dev(np.tile(a, (reps, 1, 1)))
    for _ in range(RS.SUBSTEPS):
        sim.step(1, actions=a)
    return sim


def by_replica(t, reps):
    return GD.bits(t).reshape((reps, D) + tuple(t.shape[1:]))


def build_pair(n, E_big, resident):
    assert E_big > resident, 'the launch must not fit the machine at once: %d envs, %d workgroups resident at the most' % (E_big, resident)
    small, big = new_sim(D, n), new_sim(E_big, n)
    reps = E_big // D
    # the precondition: a failure here belongs to the step kernels, not to a sensor
    bad = int((big.status != 0).sum()) + int((small.status != 0).sum())
    assert bad == 0, 'STEP KERNELS, not sensing: status is not 0 in %d envs after the six substeps' % bad
    live = GD.live_mask(small.ws_cnt, small.ws_key.shape[1])
    for name in GD.bound_fields(small):
        if name == 'scratch':
            continue
        a, b = GD.bits(getattr(small, name)), by_replica(getattr(big, name), reps)
        if name in GD.STORE_LISTS:          # the tail behind the live entries is dead
            a, b = torch.where(live, a, torch.zeros_like(a)), torch.where(live[None], b, torch.zeros_like(b))
        differ = (b != a[None]).flatten(2).any(2) if b.dim() > 2 else b != a[None]
        assert not bool(differ.any()), 'STEP KERNELS, not sensing: field %s of %d of %d envs differs from the first five after the six substeps' \
            % (name, int(differ.sum()), E_big)
    assert int(small.ws_cnt.sum(1, dtype=torch.int64).min()) > 0, 'every distinct env has contacts'
    return small, big


@pytest.fixture(scope='module')
def pair():
    t0 = time.time()
    cus = cu_count()
    W = RS.resident_workgroups(cus, 256)
    E_big = RS.batch_envs(W)
    small, big = build_pair(RS.N, E_big, W)
    print('residency: %d CUs, at most %d workgroups of 256 threads resident, %d envs of %d kilobots' % (cus, W, E_big, RS.N))
    yield small, big
    torch.cuda.synchronize()
    print('residency: the module took %.1f s on %d CUs with %d envs' % (time.time() - t0, cus, E_big))


@pytest.fixture(scope='module')
def paths_pair():
    cus = cu_count()
    W = RS.resident_by_lds(cus, 4 * RS.PATHS_BIG_GRID[0] * RS.PATHS_BIG_GRID[1])        # the plane alone: the image is larger
    E_big = RS.batch_envs(W)
    print('residency, paths above 64 KiB: %d CUs, at most %d workgroups resident, %d envs of %d kilobots' % (cus, W, E_big, RS.N_PATHS))
    return build_pair(RS.N_PATHS, E_big, W)


# ---- small against the definition -----------------------------------------------------------------------------------------
def inr_of(g):
    if not hasattr(g, '_residency_ranges'):
        g._residency_ranges = ranges(g, RS.RADIUS)
    return g._residency_ranges


def tab_of(g):
    return objects_ref.tables(g.outline())


def want_edges(g):
    src, dst, rel, count, offsets = edges_ref.restate(*state(g), RS.RADIUS)
    return src, dst, rel, offsets, count


def want_hops(g):
    seeds, inr = RS.inputs(g.num_bots)['seeds'], inr_of(g)
    envs = [hops_ref.hops_env(inr[e], seeds[e]) for e in range(D)]
    return tuple(np.stack([env[k] for env in envs]) for k in range(4))


def want_reduce(op):
    def want(g):
        return SC.check_reduce(g, inr_of(g), RS.RADIUS, op, RS.inputs(g.num_bots)['messages'], what='residency')
    return want


def want_field(g):
    v = RS.inputs(g.num_bots)
    return field_ref.restate(tab_of(g), v['field'], *state(g), v['amount'], RS.FIELD_KEEP, RS.FIELD_SPREAD, RS.FIELD_ITERS, v['field_mask'])


def want_paths(grid, suffix=''):
    def want(g):
        v = RS.inputs(g.num_bots)
        return tuple(paths_ref.restate(tab_of(g), grid[0], grid[1], v['source' + suffix], v['blocked' + suffix], (1 << g.num_objects) - 1, RS.CLEARANCE,
                                       *object_state(g))[0])
    return want


def want_light_sense(g):
    """The oracle's sensing point on the state of the sim as it is on the device, BEFORE the call moves the light."""
    torch.cuda.synchronize()
    o = O.OracleSim(O.default_config(D, g.num_bots, O.DRIVE_VELOCITY, O.LIGHT_CIRCULAR, **RS.config_kw()))
    for f in ('x', 'y', 'theta', 'light_x', 'light_y'):
        getattr(o, f)[...] = cpu(getattr(g, f))
    o.light_sense(RS.inputs(g.num_bots)['light_action'])
    return o.light_value, o.light_gx, o.light_gy, o.light_x, o.light_y


# the restatement of every output of a row, in the row's order, on the state of the sim; the shared comparers of
# tests/sensing_checks.py launch the sensor themselves and compare on the way
WANT = {
    'sense': lambda g: (SC.restate_neighbors(*state(g), RS.RADIUS, 1)[2],),
    'neighbors': lambda g: SC.check_neighbors(g, RS.RADIUS, RS.NEIGHBORS_K, 'residency')[:3],
    'edges': want_edges,
    'histogram': lambda g: SC.check_histogram(g, RS.RADIUS, RS.HIST[0], RS.HIST[1], 'residency'),
    'reduce-sum': want_reduce('sum'),
    'reduce-min': want_reduce('min'),
    'hops': want_hops,
    'clusters': lambda g: SC.check_clusters(g, inr_of(g), RS.RADIUS, what='residency'),
    'rays': lambda g: rays_ref.restate(tab_of(g), *object_state(g), RS.RAYS[0], g.cfg.bot_radius, RS.RAYS[1], nat.RAY_BOTS | nat.RAY_WALLS | nat.RAY_OBJECTS),
    'object_points': lambda g: objects_ref.restate(tab_of(g), *object_state(g))[:2],
    'grid': lambda g: (grid_ref.restate(tab_of(g), RS.GRID[0], RS.GRID[1], grid_ref.ALL, *object_state(g)),),
    'coverage': lambda g: tuple(SC.check_coverage(g, RS.GRID[0], RS.GRID[1], what='residency')),
    'field_step': want_field,
    'paths': want_paths(RS.GRID),
    'targets': lambda g: tuple(SC.check_targets(g, RS.tiled(g, 'points'), RS.TARGET_TOL, what='residency')),
    'assign': lambda g: tuple(assign_ref.restate(*state(g), RS.inputs(g.num_bots)['points'], RS.TARGET_TOL, RS.ASSIGN_CUTOFF)),
    'contacts': lambda g: SC.want_contacts(g, RS.CONTACTS_K),
    'render': lambda g: (SC.check_render(g, RS.GRID[0], RS.GRID[1], what='residency'),),
    'light_sense': want_light_sense,
    'paths-128': want_paths(RS.PATHS_BIG_GRID, '_big'),
}


def same_words(t, w):
    """The device tensor holds the array: floats by their bit patterns, integers by value."""
    a, w = cpu(t), np.asarray(w)
    assert a.shape == w.shape, (a.shape, w.shape)
    if a.dtype == np.float32:
        assert w.dtype == np.float32, w.dtype
        return np.array_equal(a.view(np.uint32), np.ascontiguousarray(w).view(np.uint32))
    assert a.dtype.kind in 'iu' and w.dtype.kind in 'iub', (a.dtype, w.dtype)
    return np.array_equal(a.astype(np.int64), w.astype(np.int64))


# ---- big against small ----------------------------------------------------------------------------------------------------
def differing_envs(name, big_t, small_t, reps):
    """The envs of big whose part of output `name` is not, bit for bit, that of env e % D of small."""
    b, s = by_replica(big_t, reps), GD.bits(small_t)
    assert tuple(b.shape[1:]) == tuple(s.shape), '%s: shapes %s and %s' % (name, tuple(big_t.shape), tuple(small_t.shape))
    d = b != s[None]
    if d.dim() > 2:
        d = d.flatten(2).any(2)
    return torch.nonzero(d.reshape(-1)).reshape(-1).tolist()


def edges_differing_envs(big_out, small_out, reps, n):
    """{output: differing envs} of the ragged edge list, per replica after removing the replica's bases: offsets[r D N] from
    the offsets, r D N from the node ids."""
    bsrc, bdst, brel, boff, bcount = big_out
    ssrc, sdst, srel, soff, scount = small_out
    rows = D * n
    found = {'count': differing_envs('count', bcount, scount, reps)}
    base = boff[:-1].reshape(reps, rows)[:, :1]
    d = (boff[:-1].reshape(reps, rows) - base != soff[:-1][None]).reshape(reps * D, n).any(1)
    found['offsets'] = torch.nonzero(d).reshape(-1).tolist()
    nnz = int(soff[-1])
    if int(boff[-1]) != reps * nnz:
        found['offsets'] = found['offsets'] or [reps * D - 1]
    if found['count'] or found['offsets']:
        return found            # the lists cannot be laid over each other
    env_of_edge = torch.div(ssrc, n, rounding_mode='floor').long()
    node_base = (torch.arange(reps, device=bsrc.device, dtype=torch.int64) * rows)[:, None]
    for name, b, s in (('src', bsrc.reshape(reps, nnz).long() - node_base, ssrc.long()), ('dst', bdst.reshape(reps, nnz).long() - node_base, sdst.long()),
                       ('rel', GD.bits(brel).reshape(reps, nnz, 4), GD.bits(srel))):
        d = b != s[None]
        if d.dim() > 2:
            d = d.any(2)
        hit = torch.zeros(reps, D, dtype=torch.int32, device=d.device)
        hit.scatter_add_(1, env_of_edge[None].expand(reps, nnz), d.to(torch.int32))
        found[name] = torch.nonzero(hit.reshape(-1)).reshape(-1).tolist()
    return found


def replica_differences(row, big_out, small_out, reps, n):
    """{output: the envs of big that differ from small}, every output of the row."""
    if row.name == 'edges':
        return edges_differing_envs(big_out, small_out, reps, n)
    assert len(big_out) == len(small_out) == len(row.outputs)
    return {name: differing_envs(name, b, s, reps) for name, b, s in zip(row.outputs, big_out, small_out)}


def report(row, found, what):
    for name, envs in found.items():
        if envs:
            e = envs[0]
            raise AssertionError('%s, %s: output %s differs in %d envs, first in env %d (replica %d, distinct env %d)' % (row.name, what, name, len(envs), e, e // D, e % D))


def per_env(row, out, n):
    """{output: [the part of each of the D envs]} of small's outputs, for the distinctness check."""
    if row.name != 'edges':
        return {name: [GD.bits(t)[e] for e in range(D)] for name, t in zip(row.outputs, out)}
    src, dst, rel, offsets, count = out
    cut = offsets[::n].tolist()
    parts = {'count': [count[e] for e in range(D)], 'offsets': [offsets[e * n:(e + 1) * n] - offsets[e * n] for e in range(D)]}
    for name, t, base in (('src', src, n), ('dst', dst, n), ('rel', GD.bits(rel), 0)):
        parts[name] = [t[cut[e]:cut[e + 1]] - e * base for e in range(D)]
    return parts


def assert_distinct(row, out, n):
    for name, parts in per_env(row, out, n).items():
        same = [(e, f) for e in range(D) for f in range(e + 1, D) if parts[e].shape == parts[f].shape and torch.equal(parts[e], parts[f])]
        if name in row.few:
            assert len(same) < D * (D - 1) // 2, '%s: output %s is the same in all %d distinct envs' % (row.name, name, D)
        else:
            assert not same, '%s: output %s does not tell the distinct envs %s apart' % (row.name, name, same)


def run_row(row, small, big):
    n, reps = small.num_bots, big.num_envs // D
    keep = [(sim, f, getattr(sim, f).clone()) for sim in (small, big) for f in ('light_x', 'light_y')]
    try:
        want = WANT[row.name](small)
        small_out = row.call(small, None)
        assert len(want) == len(small_out) == len(row.outputs)
        for name, t, w in zip(row.outputs, small_out, want):
            assert same_words(t, w), '%s: output %s of the %d distinct envs differs from the restatement' % (row.name, name, D)
        assert_distinct(row, small_out, n)
        big_out = row.call(big, None)
        for name, t in zip(row.outputs, big_out):       # (the sizes are chosen for the 4100 envs of a 256-CU device)
            assert t.numel() * t.element_size() <= OUTPUT_LIMIT or big.num_envs > 4100, '%s: output %s takes %d MiB' % (row.name, name, t.numel() * t.element_size() >> 20)
        report(row, replica_differences(row, big_out, small_out, reps, n), 'first launch')
        first = [t.clone() for t in big_out]
        again = row.call(big, big_out)
        assert all(a.data_ptr() == b.data_ptr() for name, a, b in zip(row.outputs, again, big_out) if (row.name, name) not in FRESH), \
            '%s: the second launch did not go into the tensors of the first' % row.name
        for name, a, b in zip(row.outputs, again, first):
            d = GD.bits(a) != GD.bits(b)
            assert not bool(d.any()), '%s: output %s differs in %d words between two launches into the same tensors' % (row.name, name, int(d.sum()))
    finally:
        for sim, f, t in keep:
            getattr(sim, f).copy_(t)


@pytest.mark.parametrize('row', RS.SENSORS, ids=lambda row: row.name)
def test_every_replica_equals_the_first_five(row, pair):
    run_row(row, *pair)


def test_paths_above_the_default_lds_limit(paths_pair):
    """The 128 x 128 grid: the plane alone is 64 KiB, the limit is raised and a CU takes two workgroups at the most."""
    run_row(RS.PATHS_BIG, *paths_pair)


def test_the_comparison_reaches_the_last_env(pair):
    """One kilobot of the LAST env of big moved by 0.01 m: the replica comparison of sense and neighbors reports that env and
    no other.  The kilobot is one whose count changes with the move, found on the host."""
    small, big = pair
    n, reps, last = small.num_bots, big.num_envs // D, big.num_envs - 1
    x, y = (a[D - 1] for a in state(small)[:2])
    shift = np.float32(0.01 * 25.0)
    before = reduce_ref.in_range(x, y, RS.RADIUS).sum(1)
    for i in range(n):
        moved = x.copy()
        moved[i] += shift
        if reduce_ref.in_range(moved, y, RS.RADIUS).sum(1)[i] != before[i]:
            break
    else:
        raise AssertionError('no kilobot of the last distinct env changes its count when moved by 0.01 m')
    old = big.x[last, i].clone()
    try:
        big.x[last, i] = float(moved[i])
        for name in ('sense', 'neighbors'):
            row = RS.BY_NAME[name]
            found = replica_differences(row, row.call(big, None), row.call(small, None), reps, n)
            assert all(envs in ([], [last]) for envs in found.values()), '%s: %s' % (name, {k: v[:5] for k, v in found.items()})
            assert found['count'] == [last] and (name == 'sense' or found['rel'] == [last]), '%s: %s' % (name, found)
    finally:
        big.x[last, i] = old
    for name in ('sense', 'neighbors'):
        row = RS.BY_NAME[name]
        report(row, replica_differences(row, row.call(big, None), row.call(small, None), reps, n), 'after the pose is restored')


def test_the_ragged_comparison_reaches_the_last_env(pair):
    """The same for the edge list, whose replicas are compared after their bases are removed: the best-connected kilobot of
    the last env turned by 0.1 rad leaves counts, offsets and node ids alone and changes rel in that env only."""
    small, big = pair
    n, reps, last = small.num_bots, big.num_envs // D, big.num_envs - 1
    x, y = (a[D - 1] for a in state(small)[:2])
    i = int(reduce_ref.in_range(x, y, RS.RADIUS).sum(1).argmax())
    row = RS.BY_NAME['edges']
    old = big.theta[last, i].clone()
    try:
        big.theta[last, i] = old + 0.1
        found = replica_differences(row, row.call(big, None), row.call(small, None), reps, n)
        assert found == {'count': [], 'offsets': [], 'src': [], 'dst': [], 'rel': [last]}, {k: v[:5] for k, v in found.items()}
    finally:
        big.theta[last, i] = old
    report(row, replica_differences(row, row.call(big, None), row.call(small, None), reps, n), 'after the heading is restored')
