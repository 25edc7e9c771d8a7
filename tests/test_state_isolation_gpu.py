"""Every kernel between guard bands and over poisoned dead state (tests/guarded.py), device against device.

The other GPU tests show that a plain run equals the oracle.  Here every case builds a plain KilobotSim P as they do and a
guarded one G: its bound buffers lie in one arena with a canary band of at least one env slice on both sides of each, and
before EVERY launch the dead tail of its warm-start store is made to look like live kilobot partners with impulse 1.0 and
its scratch is filled with ones or with what a launch of the twin scene (same configuration, another spawn seed) left
there.  After every launch every bound field but scratch equals P's bit for bit, of ws_key / ws_acc the live entries, and
the canaries are intact.  A kernel that stores outside its buffers, reads an entry behind an owner's list or reads a
scratch record it did not write in this launch fails here and nowhere else.  The last part runs the step kernels over LDS
that another kernel filled (kb_debug_lds)."""
import ctypes as C

import numpy as np
import pytest
import torch

from gym_kilobots_amd import _native as nat
from oracle import oracle as O
from tests import guarded as GD
from tests import overflow_scenes as OV
from tests import scenes
from tests import solver_regimes as SR
from tests import variant_census as VC
from tests.gpu_common import put_device

pytestmark = pytest.mark.gpu

HOWS = ('ones', 'stale')


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def new_sim(E, N, mode=O.DRIVE_VELOCITY, light=O.LIGHT_NONE, threads=0, **kw):
    from gym_kilobots_amd.sim import KilobotSim
    kw.setdefault('allow_sleep', 0)
    sim = KilobotSim(E, N, mode, light, debug_outputs=True, **kw)
    if threads:
        sim.block_threads = threads
    return sim


def copy_state(src, dst):
    """every bound field but scratch"""
    for name in GD.bound_fields(src):
        if name != 'scratch':
            getattr(dst, name).copy_(getattr(src, name))


def prepare(make, start, launch, how, twin, extra=0):
    """P at the start of the scene and G guarded in the same state; with how == 'stale' G's handle first runs the first
    launch of the twin scene and keeps what that left in scratch."""
    P = make()
    start(P)
    G, arena = GD.guarded_sim(make, extra)
    GD.poison_scratch(G, 'ones')
    if how == 'stale':
        twin(G)
        launch(G, 0)
        arena.check('the launch of the twin scene')
        GD.record_stale_scratch(G)
    copy_state(P, G)
    return P, G, arena


def launch_both(P, G, arena, launch, k, how, what, envs=None):
    launch(P, k)
    GD.poison_dead_store(G)
    GD.poison_scratch(G, how)
    launch(G, k)
    GD.assert_fields_equal(P, G, what, envs)
    arena.check(what)


# ---- every instantiation --------------------------------------------------------------------------------------------------
ROWS = VC.rows()
BY_INDEX = {row[1]: row for row in ROWS}


class Census:
    """make / start / twin / launch of one census row (tests/variant_census.py)"""

    def __init__(self, row, **kw):
        self.s = s = VC.scene(row)
        self.kw = dict(s.kw, **kw)
        self.steps = [(n, dev(a), dev(la)) for n, a, la in s.steps]
        self.what = VC.row_id(row)

    def make(self):
        s = self.s
        return new_sim(s.E, s.N, s.mode, s.light, threads=s.block_threads, **self.kw)

    def start(self, sim, seed_shift=0):
        sim.set_poses_m(*(VC.spawn(self.s.N, seed_shift) if seed_shift else (self.s.xy, self.s.th)))
        VC.apply_start(self.s, sim, put_device)

    def twin(self, sim):
        self.start(sim, seed_shift=1)

    def launch(self, sim, k):
        n, a, la = self.steps[k]
        sim.step(n, actions=a, light_action=la)


def run_census(row, how, **kw):
    c = Census(row, **kw)
    P, G, arena = prepare(c.make, c.start, c.launch, how, c.twin)
    # first of all: the comparison is worth nothing on another kernel
    assert G.variant_index == c.s.index and P.variant_index == c.s.index, 'the handles run instantiations %d, %d' % (G.variant_index, P.variant_index)
    for k in range(len(c.steps)):
        launch_both(P, G, arena, c.launch, k, how, '%s (%s), launch %d' % (c.what, how, k))
    assert int(P.status.max()) == 0
    assert int(P.ws_cnt.sum()) > 0


@pytest.mark.parametrize('row,how', [(row, 'ones') for row in ROWS] + [(row, 'stale') for row in ROWS if row[1] % 8 == 0],
                         ids=lambda v: v if isinstance(v, str) else VC.row_id(v))
def test_instantiation_ignores_dead_state_and_stays_in_its_buffers(row, how):
    run_census(row, how)


@pytest.mark.parametrize('index', [1, 3])
def test_the_poison_is_felt_one_entry_earlier(index):
    """The comparison can fail: the same poison impulse in the LAST LIVE entry of every env's list -- what a kernel that reads
    one entry too far would pick up -- changes the trajectory."""
    c = Census(BY_INDEX[index])
    P, G, arena = prepare(c.make, c.start, c.launch, 'ones', c.twin)
    for k in range(len(c.steps)):
        c.launch(P, k)
        GD.poison_dead_store(G)
        last = GD.live_entries(G.ws_cnt, G.ws_acc.shape[1]) - 1
        env = torch.arange(G.num_envs, device=G.device)
        G.ws_acc[env, last.clamp(min=0)] = torch.where(last >= 0, 1.0, G.ws_acc[env, last.clamp(min=0)])
        GD.poison_scratch(G, 'ones')
        c.launch(G, k)
        arena.check('%s, launch %d' % (c.what, k))
    assert not torch.equal(P.x, G.x) and not torch.equal(P.ws_acc, G.ws_acc)


# ---- scratch that is really used ------------------------------------------------------------------------------------------
SCRATCH_SCENES = [s for s in SR.SCENES if s.name in ('200-p014', '256-p010', '640-p016', '1024-p022')]


@pytest.mark.parametrize('how', HOWS)
@pytest.mark.parametrize('allow_sleep', [0, 1], ids=['nosleep', 'sleep'])
@pytest.mark.parametrize('s', SCRATCH_SCENES, ids=SR.scene_id)
def test_global_slice_regimes(s, allow_sleep, how):
    """The scenes that visit R2 and R3 (tests/test_solver_regimes_cpu.py): contacts staged in the global slice, impulses in
    the global records.  Single substeps, then the fused launch."""
    E = 2
    acts = [dev(SR.actions(E, s.N, k)) for k in range(s.substeps + 1)]
    make = lambda: new_sim(E, s.N, **SR.config_kw(s, allow_sleep))      # noqa: E731
    start = lambda sim: sim.set_poses_m(*SR.start(s, E))      # noqa: E731
    twin = lambda sim: sim.set_poses_m(*SR.start(s, E, seed=SR.SEED + 1))      # noqa: E731
    launch = lambda sim, k: sim.step(1 if k < s.substeps else SR.FUSED_SUBSTEPS, actions=acts[k])      # noqa: E731
    P, G, arena = prepare(make, start, launch, how, twin)
    band = (P.block_threads // SR.LANES, P.lds_staging_entries, P.contact_capacity)
    seen = set()
    for k in range(s.substeps + 1):
        launch_both(P, G, arena, launch, k, how, '%s sleep %d (%s), launch %d' % (s.name, allow_sleep, how, k))
        if k < s.substeps:
            seen.update(SR.classify(P.ws_cnt.cpu().numpy(), band))
    assert seen & {'R2', 'R3'}, seen
    assert int(P.status.max()) == 0


def crowd_scene(seed):
    """the scene of tests/test_parity_gpu.py::test_objects_pushed_by_a_crowd"""
    E, N = 3, 256
    xy, _ = scenes.gaussian_spawn(E, N, sigma=0.3, seed=seed)
    return xy, scenes.toward_objects_theta(xy), np.tile(scenes.CFG4_OBJECTS[None], (E, 1, 1))


@pytest.mark.parametrize('how', HOWS)
@pytest.mark.parametrize('mode', [3, 4])
def test_objects_pushed_by_a_crowd_with_staged_contacts(mode, how):
    """solver_mode 3 and 4 stage the contacts in scratch whatever their number"""
    E, N = 3, 256
    a = np.zeros((E, N, 2), np.float32)
    a[..., 0] = 0.01
    a = dev(a)

    def place(sim, seed):
        xy, th, objs = crowd_scene(seed)
        sim.set_poses_m(xy, th)
        sim.set_objects_m(objs)
    make = lambda: new_sim(E, N, num_objects=4, solver_mode=mode)      # noqa: E731
    launch = lambda sim, k: sim.step(10, actions=a)      # noqa: E731
    P, G, arena = prepare(make, lambda sim: place(sim, 61), launch, how, lambda sim: place(sim, 62))
    for k in range(5):
        launch_both(P, G, arena, launch, k, how, 'crowd, solver %d (%s), launch %d' % (mode, how, k))
    assert int(P.status.max()) == 0 and int(P.ws_cnt.sum()) > 0


@pytest.mark.parametrize('how', HOWS)
@pytest.mark.parametrize('mode', [3, 4])
def test_census_row_3_with_staged_contacts(mode, how):
    run_census(BY_INDEX[3], how, solver_mode=mode)


# ---- overflow at the edges of the batch -----------------------------------------------------------------------------------
class Overflow:
    def __init__(self, r, order=None):
        self.r, self.order = r, list(order) if order is not None else list(range(OV.E))
        self.acts = [dev(OV.actions(r, k)[self.order]) for k in range(len(r.steps))]

    def make(self):
        r = self.r
        kw = OV.config_kw(r)
        return new_sim(OV.E, r.N, r.mode, threads=r.threads, **kw)

    def start(self, sim, seed_shift=0):
        r = self.r
        sim.set_poses_m(*OV.start(r, self.order, seed_shift))
        if r.objects:
            sim.set_objects_m(OV.object_start(r))
        for name, val in OV.state(r).items():
            put_device(sim, name, val[self.order])

    def twin(self, sim):
        self.start(sim, seed_shift=1)

    def launch(self, sim, k):
        sim.step(self.r.steps[k][0], actions=self.acts[k])


@pytest.mark.parametrize('how', HOWS)
@pytest.mark.parametrize('where', ['first', 'last'])
@pytest.mark.parametrize('r', OV.CAPACITY_ROWS, ids=OV.row_id)
def test_capacity_overflow_in_the_first_and_the_last_env(r, where, how):
    """The rows of tests/test_store_overflow_gpu.py with the overflowing env at an edge of the batch, where a list or scratch
    record that leaves its slice leaves the buffer.  Only the flag of that env is specified; the others equal P's."""
    order = {'first': (1, 0, 2), 'last': (0, 2, 1)}[where]
    flagged = order.index(OV.MIDDLE)
    others = [e for e in range(OV.E) if e != flagged]
    c = Overflow(r, order)
    P, G, arena = prepare(c.make, c.start, c.launch, how, c.twin)
    for k in range(len(r.steps)):
        what = '%s, overflow %s (%s), launch %d' % (r.name, where, how, k)
        launch_both(P, G, arena, c.launch, k, how, what, envs=others)
        sp, sg = P.status.cpu().numpy(), G.status.cpu().numpy()
        assert sg[flagged] & 1 and sp[flagged] & 1, '%s: status %s, guarded %s' % (what, sp, sg)
        assert not sg[others].any(), '%s: status %s' % (what, sg)
    assert (OV.counts(P.ws_cnt.cpu().numpy())[others] >= OV.OUTER_MIN_CONTACTS).all()


@pytest.mark.parametrize('how', HOWS)
@pytest.mark.parametrize('r', [r for r in OV.SLOT_ROWS if r.N <= 200], ids=OV.row_id)
def test_slot_overflow(r, how):
    """Owners with more contacts than slots: the surplus is solved and never stored, next to a dead tail that looks alive."""
    c = Overflow(r)
    P, G, arena = prepare(c.make, c.start, c.launch, how, c.twin)
    want = np.array(r.status)
    for k in range(len(r.steps)):
        what = '%s (%s), launch %d' % (r.name, how, k)
        launch_both(P, G, arena, c.launch, k, how, what)
        sg = G.status.cpu().numpy()
        assert not (sg & 13).any(), '%s: status %s' % (what, sg)
        if k >= r.flag_by:
            assert np.array_equal(sg & 3, want), '%s: status %s, the table says %s' % (what, sg, want)


# ---- the other writers of bound buffers -----------------------------------------------------------------------------------
BOXES = dict(num_objects=2, obj_shape=[O.SHAPE_BOX] * 2 + [0] * 6, obj_nverts=[4] * 2 + [0] * 6,
             obj_verts=[[[0.075 * 25.0, 0.05 * 25.0]] + [[0.0, 0.0]] * 3] * 2 + [[[0.0, 0.0]] * 4] * 6)


def test_the_other_writers_of_bound_buffers():
    """reset, reset_envs and masked steps of the last and of the first env alone, set_actions, light_sense, poses and
    host_state on a guarded sim: 129 kilobots, two boxes, a composite light, sleeping, three envs."""
    E, N, how = 3, 129, 'ones'
    kw = dict(BOXES, allow_sleep=1, **VC._light_kw(O.LIGHT_COMPOSITE, resting=False))
    make = lambda: new_sim(E, N, O.DRIVE_VELOCITY, O.LIGHT_COMPOSITE, **kw)      # noqa: E731
    P = make()
    G, arena = GD.guarded_sim(make)
    rng = np.random.RandomState(5)
    acts = [dev(scenes.random_actions(E, N, seed=40 + k)) for k in range(4)]
    la = dev(rng.uniform(-0.02, 0.02, (E, 6)).astype(np.float32))
    objs = dev(np.concatenate([rng.uniform(-5.0, 5.0, (E, 2, 2)), rng.uniform(-3.0, 3.0, (E, 2, 1))], -1).astype(np.float32))
    lights = dev(rng.uniform(-0.2, 0.2, (E, 3, 2)).astype(np.float32))
    episode = dev(np.array([3, 1, 2], np.int32))
    only = {name: dev(np.eye(E, dtype=np.uint8)[e]) for name, e in (('last', E - 1), ('first', 0))}

    calls = [('reset', lambda s: s.reset(seed=3, std=0.1, random_theta=True)),
             ('step 0', lambda s: s.step(5, actions=acts[0], light_action=la)),
             ('step 1', lambda s: s.step(1, actions=acts[1]))]
    for name in ('last', 'first'):
        calls += [('reset_envs, %s env' % name, lambda s, m=only[name]: s.reset_envs(m, seed=4, std=0.1, random_theta=True, episode=episode,
                                                                                    objects=objs, lights=lights)),
                  ('masked step, %s env' % name, lambda s, m=only[name]: s.step(3, actions=acts[2], light_action=la, env_mask=m))]
    calls += [('set_actions', lambda s: s.set_actions(acts[3])),
              ('light_sense', lambda s: s.light_sense(la)),
              ('step 2', lambda s: s.step(2))]
    for what, call in calls:
        call(P)
        GD.poison_dead_store(G)
        GD.poison_scratch(G, how)
        call(G)
        GD.assert_fields_equal(P, G, what)
        arena.check(what)
        # (an env that hits a staging limit, status bit 2, drops contacts in the order its atomics fall: nothing to compare)
        assert int(P.status.max()) == 0, '%s: status %s' % (what, P.status.cpu().numpy())
    assert int(P.ws_cnt.sum(1).min()) > 0, 'every env has contacts'
    for what in ('poses', 'object_poses'):
        assert torch.equal(GD.bits(getattr(P, what)()), GD.bits(getattr(G, what)())), what
        arena.check(what)
    for a, b in zip(P.host_state(), G.host_state()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), 'host_state'
    GD.assert_fields_equal(P, G, 'after the read-backs')
    arena.check('host_state')


# ---- sensing outputs between bands ----------------------------------------------------------------------------------------
RADIUS = 0.07


def _reduce(op):
    def call(sim, out):
        values = torch.linspace(-2.0, 2.0, sim.num_envs * sim.num_bots * 8, device=sim.device).reshape(sim.num_envs, sim.num_bots, 8).contiguous()
        return sim.neighbor_reduce(values, RADIUS, op=op, out=out, count=True)
    return call


def _hops(sim, out):
    seeds = (torch.arange(sim.num_bots, device=sim.device) % 7 == 0)[None, :].expand(sim.num_envs, -1).contiguous()
    return sim.hops(seeds, RADIUS, parent=True, root=True, stats=True, out=out)


SENSORS = {
    'sense': lambda sim, out: (sim.sense(RADIUS, out=out),),
    'neighbors-k1': lambda sim, out: sim.neighbors(RADIUS, 1, out=out),
    'neighbors-k16': lambda sim, out: sim.neighbors(RADIUS, 16, out=out),
    'histogram-8x8': lambda sim, out: sim.neighbor_histogram(RADIUS, 8, 8, out=out, count=True),
    'reduce-sum': _reduce('sum'), 'reduce-min': _reduce('min'), 'reduce-max': _reduce('max'),
    'hops': _hops,
    'object_points': lambda sim, out: sim.object_points(out=out),
    'grid-5': lambda sim, out: (sim.occupancy_grid(5, 3, ('count', 'flow', 'objects'), out=out),),
    'grid-128': lambda sim, out: (sim.occupancy_grid(128, 96, ('count', 'flow', 'objects'), out=out),),
    'contacts-k16': lambda sim, out: sim.contacts(16, out=out),
    'render-7': lambda sim, out: (sim.render(7, 5, out=out),),
    'render-64': lambda sim, out: (sim.render(64, 48, out=out),),
    'rays-32': lambda sim, out: sim.rays(0.2, 32, out=out),
}


@pytest.fixture(scope='module', params=[1, 129], ids=['n1', 'n129'])
def sensing_pair(request):
    """(P, G, arena): two envs of N kilobots around two boxes after six substeps, so that the store has contacts; G is
    guarded, and its arena has room for every output of the sensing tests"""
    E, N = 2, request.param
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.1, seed=17)
    objs = np.tile(VC.OBJECTS[None], (E, 1, 1))
    make = lambda: new_sim(E, N, **BOXES)      # noqa: E731
    P = make()
    P.set_poses_m(xy, th)
    P.set_objects_m(objs)
    a = dev(scenes.random_actions(E, N, seed=18))
    for _ in range(6):
        P.step(1, actions=a)
    G, arena = GD.guarded_sim(make, extra=8 << 20)
    copy_state(P, G)
    assert int(P.status.max()) == 0 and (N == 1 or int(P.ws_cnt.sum(1).min()) > 0)
    return P, G, arena


def take_like(arena, tensors, E, name):
    return tuple(arena.take(t.shape, t.dtype, t.numel() * t.element_size() // E, '%s output %d' % (name, i)) for i, t in enumerate(tensors))


def poison_for_sensing(G):
    GD.poison_dead_store(G)
    if G.num_bots >= 2:         # (the word 1 is a kilobot index only then)
        GD.poison_scratch(G, 'ones')


@pytest.mark.parametrize('name', sorted(SENSORS))
def test_sensing_outputs_between_bands(name, sensing_pair):
    P, G, arena = sensing_pair
    call = SENSORS[name]
    fresh = [t for t in call(P, None) if t is not None]
    out = take_like(arena, fresh, P.num_envs, name)
    poison_for_sensing(G)
    got = [t for t in call(G, out if len(out) > 1 else out[0]) if t is not None]
    assert len(got) == len(fresh) and all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    for i, (a, b) in enumerate(zip(fresh, got)):
        assert torch.equal(GD.bits(a), GD.bits(b)), '%s: output %d differs' % (name, i)
    arena.check(name)
    GD.assert_fields_equal(P, G, name)
    if name in ('sense', 'contacts-k16') and P.num_bots > 1:
        assert bool(fresh[0].ne(-1 if name != 'sense' else 0).any()), 'the scene has neighbours and contacts'


def test_edges_at_and_below_their_capacity(sensing_pair):
    """capacity = nnz exactly: the last edge fills the last slot; capacity = nnz - 1: it is dropped"""
    P, G, arena = sensing_pair
    nnz = P.edges(RADIUS).nnz
    assert (nnz > 0) == (P.num_bots > 1)
    for cap in [nnz] + ([nnz - 1] if nnz > 0 else []):
        fresh = P.edges(RADIUS, capacity=cap)
        out = take_like(arena, (fresh.src, fresh.dst, fresh.rel), P.num_envs, 'edges (capacity %d)' % cap)
        poison_for_sensing(G)
        got = G.edges(RADIUS, capacity=cap, out=out)
        what = 'edges, capacity %d of %d' % (cap, nnz)
        assert got.src.data_ptr() == out[0].data_ptr() and got.dst.data_ptr() == out[1].data_ptr() and got.rel.data_ptr() == out[2].data_ptr()
        for f in ('src', 'dst', 'rel', 'offsets', 'count'):
            assert torch.equal(GD.bits(getattr(fresh, f)), GD.bits(getattr(got, f))), '%s: %s differs' % (what, f)
        assert int(fresh.nnz) == nnz and int(got.nnz) == nnz
        arena.check(what)
    GD.assert_fields_equal(P, G, 'edges')


# ---- a fresh handle continues the run -------------------------------------------------------------------------------------
HANDOVER = 20
MIXED_ROW = 164


@pytest.mark.parametrize('index', [1, 3, 9, MIXED_ROW])
def test_a_fresh_handle_continues_the_run(index):
    """Neither the handle nor scratch carries state from launch to launch: after 20 launches the bound fields but scratch go
    into a newly created sim, which runs the remaining launches over a poisoned store tail and scratch like the first."""
    c = Census(BY_INDEX[index])
    P = c.make()
    c.start(P)
    for k in range(HANDOVER):
        c.launch(P, k)
    F, arena = GD.guarded_sim(c.make)
    assert F.variant_index == index and P.variant_index == index
    copy_state(P, F)
    assert int(P.ws_cnt.sum(1).min()) > 0, 'the store that is handed over has entries'
    for k in range(HANDOVER, len(c.steps)):
        launch_both(P, F, arena, c.launch, k, 'ones', '%s, fresh handle, launch %d' % (c.what, k))
    assert int(P.status.max()) == 0


# ---- LDS that something else filled ---------------------------------------------------------------------------------------
LDS_WORD = 1            # a kilobot index, a small count, a finite float
LDS_WORDS_PER_CU = 160 * 1024 // 4


@pytest.fixture(scope='module')
def lds_share():
    """The share of the LDS words that a kernel finds as the kernel before it left them: kb_debug_lds fills, then counts."""
    lib = nat.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    counts = torch.zeros(2, dtype=torch.int64, device='cuda')
    nat.check(lib.kb_debug_lds(0, LDS_WORD, None, stream), 'kb_debug_lds')
    nat.check(lib.kb_debug_lds(1, LDS_WORD, C.c_void_p(counts.data_ptr()), stream), 'kb_debug_lds')
    hit, looked = (int(v) for v in counts.cpu())
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    assert looked == 2 * cus * LDS_WORDS_PER_CU, (looked, cus)
    print('kb_debug_lds: %d of %d LDS words survive from one kernel to the next (%.4f)' % (hit, looked, hit / looked))
    return hit / looked


def test_lds_probe_counts_what_it_is_told(lds_share):
    assert 0.0 <= lds_share <= 1.0


@pytest.mark.parametrize('index', [1, 3, 7, 9, 160, MIXED_ROW])
def test_step_kernels_over_lds_that_another_kernel_filled(index, lds_share):
    """G's every launch follows a kernel that wrote 1 into every LDS word of every CU; P's follows what it always follows.  A
    word that a step kernel reads before it writes it differs between the two."""
    if lds_share < 0.5:
        pytest.skip('only %.4f of the LDS words survive from one kernel to the next on this device: the comparison would be vacuous' % lds_share)
    lib = nat.load()
    c = Census(BY_INDEX[index])
    P, G = c.make(), c.make()
    c.start(P)
    c.start(G)
    assert G.variant_index == index and P.variant_index == index
    for k in range(len(c.steps)):
        c.launch(P, k)
        nat.check(lib.kb_debug_lds(0, LDS_WORD, None, G._stream()), 'kb_debug_lds')
        c.launch(G, k)
        GD.assert_fields_equal(P, G, '%s over filled LDS, launch %d' % (c.what, k))
    assert int(P.status.max()) == 0 and int(P.ws_cnt.sum()) > 0
