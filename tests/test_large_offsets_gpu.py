"""Every kernel where byte offsets pass 2^31 and 2^32 (tests/offset_scenes.py has the sizes, tests/test_large_offsets_cpu.py
shows that they follow from the ABI constants and that no scene is vacuous).

D = 5 distinct envs are tiled to E envs.  Per row: the distinct envs equal the restatement (sensing, field, render) or the
oracle (step) bit for bit; every replica equals its distinct env, compared on the device in blocks of envs; the probe envs --
around 2^31 bytes, around 2^32 bytes, the last -- are pulled to the host and compared with the restatement directly.  Every
output under test, and the scratch of the step rows, is a view that begins 2^31 bytes into an allocation full of the
sentinel byte: an offset truncated to 32 bits lands in the tensor, where the comparisons find it, one sign-extended from 32
bits lands in the band, which is checked after every launch.  Two negative controls change something of the LAST env and
require that the comparison names that env and no other: the harness itself reaches past 4 GiB.  No tolerances anywhere.

A row is skipped only where the device has less free memory than the row needs plus a quarter."""
import time

import numpy as np
import pytest
import torch

from tests import contacts_ref
from tests import contacts_scenes
from tests import edges_ref
from tests import guarded as GD
from tests import objects_ref
from tests import offset_scenes as OS
from tests import reduce_ref
from tests import reset_envs_ref as R
from tests import residency_scenes as RS
from tests import sensing_checks as SC
from tests import test_sensing_residency_gpu as RG
from tests.gpu_common import OBJ_FIELDS, OBJECT_STATE, assert_same, assert_ws_same, cpu, dev

pytestmark = pytest.mark.gpu

D, B31, B32 = OS.D, OS.B31, OS.B32
BLOCK_BYTES = 1 << 30           # no fill or band check touches more bytes in one op
BLOCK_ELEMS = 1 << 27           # ... and no comparison more elements
I32, F32, U8 = torch.int32, torch.float32, torch.uint8


_fault = []


@pytest.fixture(autouse=True)
def nothing_is_launched_after_a_fault():
    """A device fault is sticky: the synchronisation after the test that met it raises.  Nothing of this module runs after it."""
    assert not _fault, 'an earlier test of this module met a device fault (%s): nothing more is launched' % _fault[0]
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        _fault.append(str(e).splitlines()[0])


# ---- memory -----------------------------------------------------------------------------------------------------------------
def require(need, what):
    """Skip unless the device has `need` bytes and a quarter more free."""
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < need * OS.HEADROOM:
        pytest.skip('%s needs %d bytes and a quarter more, %d are free' % (what, need, free))


def nbytes(t):
    return t.numel() * t.element_size()


class Banded:
    """A tensor that begins FRONT_BAND bytes into an allocation full of the sentinel byte."""

    def __init__(self, shape, dtype, device, name):
        shape = tuple(int(s) for s in shape)
        n = int(np.prod(shape, dtype=np.int64)) * torch.empty(0, dtype=dtype).element_size()
        self.name = name
        self.buf = torch.empty(OS.FRONT_BAND + n, dtype=U8, device=device)
        self.fill()
        self.view = self.buf[OS.FRONT_BAND:].view(dtype).view(shape)
        assert self.view.data_ptr() % 16 == 0 and self.view.is_contiguous() and self.view.data_ptr() - self.buf.data_ptr() == OS.FRONT_BAND

    def fill(self):
        for a in range(0, self.buf.numel(), BLOCK_BYTES):
            self.buf[a:a + BLOCK_BYTES].fill_(OS.SENTINEL)

    def changed(self):
        """0-dim int64 on the device: bytes of the band that are no longer the sentinel"""
        bad = torch.zeros((), dtype=torch.int64, device=self.buf.device)
        for a in range(0, OS.FRONT_BAND, BLOCK_BYTES):
            bad += (self.buf[a:min(a + BLOCK_BYTES, OS.FRONT_BAND)] != OS.SENTINEL).sum()
        return bad


def check_bands(bands, what):
    """Every front band in one read-back; GuardError names the tensor and how far in front of it the nearest changed byte is."""
    bands = list(bands)
    if not bands:
        return
    bad = torch.stack([b.changed() for b in bands]).tolist()
    for b, n in zip(bands, bad):
        if n:
            for a in range(0, OS.FRONT_BAND, BLOCK_BYTES):
                at = torch.nonzero(b.buf[a:min(a + BLOCK_BYTES, OS.FRONT_BAND)] != OS.SENTINEL)
                if at.numel():
                    pos = a + int(at.max())
            raise GD.GuardError('%s: %d bytes of the front band of %s changed, the nearest %d bytes in front of it' % (what, n, b.name, OS.FRONT_BAND - pos))


# ---- comparisons ------------------------------------------------------------------------------------------------------------
def replica_differences(t, mask=None, head=None):
    """The envs of t [E, ...] whose bits are not those of env e % D of head (None: the first D of t), block by block.  mask
    [D, ...] bool: the elements that count."""
    b = GD.bits(t)
    E = b.shape[0]
    assert E % D == 0
    head = b[:D] if head is None else GD.bits(head)
    blk = max(D, BLOCK_ELEMS // max(1, b[0].numel()) // D * D)
    found = []
    for e0 in range(0, E, blk):
        part = b[e0:e0 + blk]
        d = part.reshape((-1, D) + tuple(b.shape[1:])) != head[None]
        if mask is not None:
            d &= mask[None]
        if d.dim() > 2:
            d = d.flatten(2).any(2)
        found.append(torch.nonzero(d.reshape(-1)).reshape(-1) + e0)
    return torch.cat(found).tolist()


def no_differences(found, what):
    assert not found, '%s differs from its distinct env in %d envs, first in env %d (replica %d, scene %d)' % (what, len(found), found[0], found[0] // D, found[0] % D)


def tile_into(dst, src):
    """dst [E, ...] on the device = src [D, ...] tiled, block by block"""
    src = src if torch.is_tensor(src) else dev(src)
    blk = max(D, BLOCK_ELEMS // max(1, src[0].numel()) // D * D)
    for e0 in range(0, dst.shape[0], blk):
        part = dst[e0:e0 + blk]
        part.reshape((-1,) + tuple(src.shape)).copy_(src[None].expand((part.shape[0] // D,) + tuple(src.shape)))
    return dst


def hold(row_name, names, outs, want, probes, what):
    """The distinct envs and the probe envs against the restatement, every replica against its distinct env."""
    assert len(names) == len(outs) == len(want)
    for name, t, w in zip(names, outs, want):
        assert RG.same_words(t[:D], w), '%s: output %s of the %d distinct envs differs from the restatement' % (what, name, D)
        for p in probes:
            assert RG.same_words(t[p:p + 1], np.asarray(w)[p % D][None]), '%s: output %s of probe env %d differs from the restatement of scene %d' % (what, name, p, p % D)
        no_differences(replica_differences(t), '%s: output %s' % (what, name))


# ---- row 3, 4 and 6: the sensing handle ---------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def big():
    """The residency scene at 1024 kilobots tiled to 16390 envs, as spawned (offset_scenes.sensing_oracle says why)."""
    from gym_kilobots_amd.sim import KilobotSim
    E, N, reps = OS.E_SENSE, OS.N_SENSE, OS.E_SENSE // D
    require(OS.sensing_sim_need(E, N), 'the sensing handle of %d envs' % E)
    t0 = time.time()
    xy, th, objs, _ = RS.spawn(N)
    sim = KilobotSim(E, N, OS.O.DRIVE_VELOCITY, OS.O.LIGHT_CIRCULAR, debug_outputs=True, **RS.config_kw())
    sim.set_poses_m(np.tile(xy, (reps, 1, 1)), np.tile(th, (reps, 1)))
    sim.set_objects_m(np.tile(objs, (reps, 1, 1)))
    sim.light_x.copy_(dev(np.tile(RS.LIGHTS_M[:, 0], reps)))
    sim.light_y.copy_(dev(np.tile(RS.LIGHTS_M[:, 1], reps)))
    torch.cuda.synchronize()
    o = OS.sensing_oracle()
    st = tuple(cpu(getattr(sim, f)[:D]) for f in OBJECT_STATE)
    for f, a in zip(OBJECT_STATE, st):
        assert np.array_equal(a.view(np.uint32), getattr(o, f).view(np.uint32)), 'field %s of the distinct envs is not what the oracle holds' % f
        no_differences(replica_differences(getattr(sim, f)), 'field ' + f)
    print('large offsets: the sensing handle, %d envs of %d kilobots, took %.1f s' % (E, N, time.time() - t0))
    yield sim, st, objects_ref.tables(sim.outline())
    sim.close()


def _field_call(sim, outs):
    field, sense = outs
    tile_into(field, OS.field_inputs()[0])
    amount = tile_into(torch.empty(sim.num_envs, sim.num_bots, OS.FIELD_CHANNELS, dtype=F32, device=sim.device), OS.field_inputs()[1])
    mask = dev(OS.FIELD_MASK).repeat(sim.num_envs // D)
    sim.field_step(field, amount, OS.FIELD_KEEP, OS.FIELD_SPREAD, OS.FIELD_ITERS, mask, out=sense)
    return field, sense


_N = OS.N_SENSE
# name -> (shape and dtype of every output without the env axis, call(sim, outs) -> the outputs)
LAUNCH = {
    'neighbors': ([((_N, OS.NEIGHBORS_K), I32), ((_N, OS.NEIGHBORS_K, 4), F32), ((_N,), I32)], lambda sim, outs: sim.neighbors(OS.RADIUS, OS.NEIGHBORS_K, out=outs)),
    'histogram': ([((_N,) + OS.HIST, F32), ((_N,), I32)], lambda sim, outs: sim.neighbor_histogram(OS.RADIUS, OS.HIST[0], OS.HIST[1], out=outs, count=True)),
    'field_step': ([((OS.FIELD_CHANNELS, OS.GRID[1], OS.GRID[0]), F32), ((_N, OS.FIELD_CHANNELS, 4), F32)], _field_call),
    'grid': ([((OS.GRID_CHANNELS, OS.GRID[1], OS.GRID[0]), F32)], lambda sim, outs: (sim.occupancy_grid(OS.GRID[0], OS.GRID[1], ('count', 'flow', 'objects'), out=outs[0]),)),
    'rays': ([((_N, OS.RAYS[1]), F32), ((_N, OS.RAYS[1]), I32)], lambda sim, outs: sim.rays(OS.RAYS[0], OS.RAYS[1], out=outs)),
    'object_points': ([((_N, RS.BOXES['num_objects'], 4), F32), ((_N, 4), F32)], lambda sim, outs: sim.object_points(out=outs)),
}
SENSING_ROWS = [r for r in OS.CROSSING if r.name != 'render'] + [OS.OBJECT_POINTS]


def banded_outputs(row, sim):
    shapes = LAUNCH[row.name][0]
    E = sim.num_envs
    bands = [Banded((E,) + s, dt, sim.device, '%s output %s' % (row.name, name)) for (s, dt), (name, _) in zip(shapes, row.outputs)]
    for b, (name, row_bytes) in zip(bands, row.outputs):
        assert nbytes(b.view) == E * row_bytes, '%s: output %s has %d bytes per env, the table says %d' % (row.name, name, nbytes(b.view) // E, row_bytes)
    return bands


def launch_sensing(row, sim):
    bands = banded_outputs(row, sim)
    views = tuple(b.view for b in bands)
    got = LAUNCH[row.name][1](sim, views)
    torch.cuda.synchronize()
    assert all(g.data_ptr() == v.data_ptr() for g, v in zip(got, views)), '%s: the launch did not go into the banded tensors' % row.name
    return bands, views


@pytest.mark.parametrize('row', SENSING_ROWS, ids=lambda r: r.name)
def test_sensing_row(row, big):
    sim, st, tab = big
    E = sim.num_envs
    sizes = dict(row.outputs)
    require(sum(OS.FRONT_BAND + E * b for b in sizes.values()) + E * 4 * OS.N_SENSE * OS.FIELD_CHANNELS, row.name)
    t0 = time.time()
    fill = np.full((D, OS.N_SENSE, OS.FIELD_CHANNELS, 4), OS.SENTINEL_WORD, np.uint32).view(np.float32)     # the rows of the masked scene stay what they were
    want = OS.want(row.name, tab, st, fill)
    t1 = time.time()
    bands, outs = launch_sensing(row, sim)
    t2 = time.time()
    probes = OS.probes(sizes[row.claims], E)
    assert OS.reached(sizes[row.claims], E) == (row.boundary if row is not OS.OBJECT_POINTS else None)
    hold(row.name, [n for n, _ in row.outputs], outs, want, probes, row.name)
    check_bands(bands, row.name)
    if row.name == 'field_step':
        off = [e for e in range(D) if not OS.FIELD_MASK[e]]
        assert off and bool((outs[1][off].view(I32) == OS.SENTINEL_WORD).all()), 'field_step: the sense rows of a masked env were written'
    print('large offsets, %s: %d envs, %s, probes %s; restatement %.1f s, allocation and launch %.1f s, comparison %.1f s'
          % (row.name, E, ', '.join('%s %.2f GB' % (n, E * b / 1e9) for n, b in row.outputs), probes, t1 - t0, t2 - t1, time.time() - t2))


def test_the_comparison_of_neighbors_reaches_the_last_env(big):
    """Negative control: one kilobot of the LAST env -- above 2^32 bytes of rel -- moved by 0.01 m; the comparison names that env
    and no other.  The kilobot is one whose count changes with the move, found on the host."""
    sim, st, tab = big
    row = OS.CROSSING_BY_NAME['neighbors']
    E, last = sim.num_envs, sim.num_envs - 1
    require(OS.sensing_need(row), 'neighbors, negative control')
    assert last * dict(row.outputs)['rel'] >= B32
    x, y = st[0][last % D], st[1][last % D]
    before = reduce_ref.in_range(x, y, OS.RADIUS).sum(1)
    for i in range(OS.N_SENSE):
        moved = x.copy()
        moved[i] += np.float32(0.01 * 25.0)
        if reduce_ref.in_range(moved, y, OS.RADIUS).sum(1)[i] != before[i]:
            break
    else:
        raise AssertionError('no kilobot of the last env changes its count when moved by 0.01 m')
    old = sim.x[last, i].clone()
    try:
        sim.x[last, i] = float(moved[i])
        bands, outs = launch_sensing(row, sim)
    finally:
        sim.x[last, i] = old
    found = {name: replica_differences(t) for (name, _), t in zip(row.outputs, outs)}
    assert all(envs in ([], [last]) for envs in found.values()) and found['count'] == [last] and found['rel'] == [last], {k: v[:5] for k, v in found.items()}
    check_bands(bands, 'neighbors, negative control')


def test_edges_pass_their_boundaries(big):
    """Row 4: nnz >= 2^28 edges plus one env's, so rel passes 2^32 bytes and src and dst 2^30; the row pointer from torch.cumsum as
    KilobotSim.edges makes it; per replica after removing its bases; with capacity = nnz, then nnz - 1."""
    sim, st, tab = big
    E, N, reps = sim.num_envs, sim.num_bots, sim.num_envs // D
    x, y, th = st[:3]
    sums = {Rm: [int(reduce_ref.in_range(x[e], y[e], Rm).sum()) for e in range(D)] for Rm in OS.EDGE_RADII}
    radius, nnz = OS.edges_radius(sums, E)
    require(OS.edges_need(nnz), 'edges')
    t0 = time.time()
    wsrc, wdst, wrel, wcount, woff = edges_ref.restate(x, y, th, radius)
    m, rows = len(wsrc), D * N
    assert m * reps == nnz and 16 * nnz > B32 and 4 * nnz > 1 << 30
    small = tuple(dev(a) for a in (wsrc, wdst, wrel, woff, wcount.astype(np.int32)))
    bands = [Banded(s, dt, sim.device, 'edges output ' + name) for name, s, dt in (('src', (nnz,), I32), ('dst', (nnz,), I32), ('rel', (nnz, 4), F32))]
    # the replicas that hold the first edge above 2^31 and above 2^32 bytes of rel, the one after each, and the last
    probes = sorted({reps - 1} | {r for b in (B31, B32) for r in (b // 16 // m, b // 16 // m + 1) if r < reps})
    t1 = time.time()
    for capacity in (nnz, nnz - 1):
        what = 'edges, capacity %d of %d' % (capacity, nnz)
        for b in bands:
            b.fill()
        e = sim.edges(radius, capacity=capacity, out=tuple(b.view[:capacity] for b in bands))
        torch.cuda.synchronize()
        assert int(e.nnz) == nnz and e.src.data_ptr() == bands[0].view.data_ptr() and e.rel.data_ptr() == bands[2].view.data_ptr()
        check_bands(bands, what)
        whole = reps if capacity == nnz else reps - 1       # the replicas that are whole
        step = max(1, BLOCK_ELEMS // (4 * m))
        for r0 in range(0, whole, step):
            r1 = min(r0 + step, whole)
            part = (e.src[r0 * m:r1 * m] - r0 * rows, e.dst[r0 * m:r1 * m] - r0 * rows, e.rel[r0 * m:r1 * m], e.offsets[r0 * rows:r1 * rows + 1] - e.offsets[r0 * rows],
                    e.count[r0 * D:r1 * D])
            found = RG.edges_differing_envs(part, small, r1 - r0, N)
            for name, envs in found.items():
                assert not envs, '%s: %s differs in %d envs, first in env %d' % (what, name, len(envs), envs[0] + r0 * D)
        for r in probes:
            n = m if r < reps - 1 else m - (nnz - capacity)
            lo = r * m
            assert np.array_equal(cpu(e.src[lo:lo + n]).astype(np.int64) - r * rows, wsrc[:n]) and np.array_equal(cpu(e.dst[lo:lo + n]).astype(np.int64) - r * rows, wdst[:n]), \
                '%s: the node ids of replica %d differ from the restatement' % (what, r)
            assert np.array_equal(cpu(e.rel[lo:lo + n]).view(np.uint32), wrel[:n].view(np.uint32)), '%s: rel of replica %d differs from the restatement' % (what, r)
        assert int(e.offsets[-1]) == nnz and np.array_equal(cpu(e.offsets[:rows + 1]), woff)
        if capacity < nnz:      # the last row is cut: nothing is written at or beyond the capacity
            for b in bands:
                assert bool((b.view[capacity:].reshape(-1).view(I32) == OS.SENTINEL_WORD).all()), '%s: %s was written at its capacity' % (what, b.name)
    print('large offsets, edges: radius %g, %d edges, rel %.2f GB, src and dst %.2f GB, replicas probed %s; restatement %.1f s, launches and comparison %.1f s'
          % (radius, nnz, 16 * nnz / 1e9, 4 * nnz / 1e9, probes, t1 - t0, time.time() - t1))


def _poses(sim, out):
    return (sim.poses(),)


def _set_actions(sim, out):
    sim.set_actions(dev(RS.spawn(sim.num_bots)[3]).repeat(sim.num_envs // D, 1, 1))
    return sim.v, sim.w


def test_the_entries_that_cannot_cross_run_on_the_largest_batch(big):
    """Row 6: their rows stay below 128 KiB per env, so no batch is built for them; on this one they read the state of envs
    above index 16384 and launch 16390 x bands workgroups.  The replica relation only."""
    sim, st, tab = big
    t0 = time.time()
    keep = [(f, getattr(sim, f).clone()) for f in ('light_x', 'light_y', 'v', 'w')]
    rows = [RS.BY_NAME[name] for name in OS.CANNOT_CROSS if name in RS.BY_NAME]
    rows += [RS.Row('poses', 'poses', ('poses',), _poses, ()), RS.Row('set_actions', 'set_actions', ('v', 'w'), _set_actions, ())]
    assert sorted({r.name for r in rows} | {'host_state', 'reset'}) == sorted(OS.CANNOT_CROSS)
    try:
        for row in rows:
            outs = row.call(sim, None)
            torch.cuda.synchronize()
            for name, t in zip(row.outputs, outs):
                assert nbytes(t) // sim.num_envs <= OS.CANNOT_CROSS[row.name][1], '%s: output %s has %d bytes per env' % (row.name, name, nbytes(t) // sim.num_envs)
                no_differences(replica_differences(t), '%s: output %s' % (row.name, name))
        for name, a in zip(('poses', 'objects', 'status'), sim.host_state()):
            t = np.ascontiguousarray(a).view(np.uint32).reshape((-1, D) + a.shape[1:])
            assert np.array_equal(t, np.broadcast_to(t[:1], t.shape)), 'host_state: %s differs between replicas' % name
    finally:
        for f, t in keep:
            getattr(sim, f).copy_(t)
    print('large offsets, the %d entries that cannot cross: %.1f s' % (len(rows) + 1, time.time() - t0))


# ---- row 5: render ------------------------------------------------------------------------------------------------------------
def test_render_passes_2_32_bytes():
    """64 kilobots, 350 envs, 2048 x 2048 with all layers.  The restatement of a whole frame takes seven seconds: the distinct and
    the probe envs are held to it on 64 rows at the top, in the middle and at the bottom of the frame, every byte of every frame
    through the replica relation.  Negative control: one byte of the last env's frame flipped after the launch."""
    row = OS.CROSSING_BY_NAME['render']
    E, side = OS.E_RENDER, OS.RENDER_SIDE
    require(OS.sensing_need(row) + OS.sensing_sim_need(E, OS.RENDER_N), 'render')
    t0 = time.time()
    sim = RG.new_sim(E, OS.RENDER_N)
    torch.cuda.synchronize()
    assert int((sim.status != 0).sum()) == 0
    st = tuple(cpu(getattr(sim, f)[:D]) for f in OBJECT_STATE)
    for f in OBJECT_STATE + ('light_x', 'light_y'):
        no_differences(replica_differences(getattr(sim, f)), 'STEP KERNELS, not render: field ' + f)
    want = OS.want_render_bands(objects_ref.tables(sim.outline()), st, np.stack([cpu(sim.light_x[:D]), cpu(sim.light_y[:D])], 1), sim.cfg.bot_radius)
    t1 = time.time()
    band = Banded((E, side, side, 3), U8, sim.device, 'render output rgb')
    assert nbytes(band.view) == E * OS.RENDER_ROW
    got = sim.render(side, side, out=band.view)
    torch.cuda.synchronize()
    t2 = time.time()
    assert got.data_ptr() == band.view.data_ptr()
    check_bands([band], 'render')
    rows = dev(np.array(OS.RENDER_BANDS))
    probes = OS.probes(OS.RENDER_ROW, E)
    assert probes == [170, 171, 341, 342, 349]
    for e in list(range(D)) + probes:
        assert np.array_equal(cpu(got[e][rows]), want[e % D]), 'render: the bands of env %d differ from the restatement of scene %d' % (e, e % D)
    assert not bool((got[:D] == OS.SENTINEL).all(-1).any()), 'render: a pixel of the distinct envs still holds the sentinel'
    no_differences(replica_differences(got), 'render: output rgb')
    last = E - 1
    assert last * OS.RENDER_ROW >= B32
    at = (last, side - 1, side - 1, 2)          # the last byte of the tensor
    got[at] ^= 0xFF
    try:
        assert replica_differences(got) == [last], 'render, negative control: the byte comparison does not name the last env alone'
    finally:
        got[at] ^= 0xFF
    sim.close()
    print('large offsets, render: %d envs, rgb %.2f GB, probes %s; the scene and the restatement of the bands %.1f s, allocation and launch %.1f s, comparison %.1f s'
          % (E, E * OS.RENDER_ROW / 1e9, probes, t1 - t0, t2 - t1, time.time() - t2))


# ---- row 1 and 2: the step kernels --------------------------------------------------------------------------------------------
class Envs:
    """The envs `envs` of a KilobotSim as gpu_common's comparers take a sim."""

    def __init__(self, sim, envs):
        idx = torch.as_tensor(list(envs), device=sim.device)
        for name in GD.bound_fields(sim):
            if name != 'scratch':
                setattr(self, name, getattr(sim, name)[idx])


class OracleRows:
    """The rows `rows` of the state arrays of an OracleSim as gpu_common's comparers take an oracle."""

    def __init__(self, o, rows):
        self.cap = o.cap
        for name in R.STATE_FIELDS:
            a = getattr(o, name, None)
            if isinstance(a, np.ndarray) and a.ndim and a.shape[0] == D:
                setattr(self, name, a[list(rows)])


def replicas_hold(gsim, what, envs=None):
    """Every bound field but scratch, of the store lists the live entries: envs [0, envs) against the first D."""
    E = gsim.num_envs if envs is None else envs
    cap = gsim.ws_key.shape[1]
    width = max(1, int(GD.live_entries(gsim.ws_cnt[:D], cap).max()))
    live = GD.live_mask(gsim.ws_cnt[:D], cap)[:, :width]
    for name in GD.bound_fields(gsim):
        if name == 'scratch':
            continue
        t = getattr(gsim, name)[:E]
        found = replica_differences(t[:, :width], live) if name in GD.STORE_LISTS else replica_differences(t)
        no_differences(found, '%s: field %s' % (what, name))


def held_to_the_oracle(osim, gsim, envs, fields, what):
    part, rows = Envs(gsim, envs), OracleRows(osim, [e % D for e in envs])
    assert_same(rows, part, what, fields)
    assert_ws_same(rows, part, what)


def contacts_hold(gsim, groups, replicas, what):
    """kb_sense_contacts with all outputs into banded tensors: the envs of `groups` against contacts_ref on their own store,
    envs [0, replicas) against the first D."""
    E, N, M, k = gsim.num_envs, gsim.num_bots, gsim.num_objects, OS.CONTACTS_K
    shapes = [('partner', (E, N, k), I32), ('impulse', (E, N, k), F32), ('touch', (E, N, 4), F32)] + ([('obj', (E, M, 2), F32)] if M else [])
    bands = [Banded(s, dt, gsim.device, 'contacts output ' + name) for name, s, dt in shapes]
    got = gsim.contacts(k, out=tuple(b.view for b in bands))
    torch.cuda.synchronize()
    check_bands(bands, what)
    body = contacts_scenes.fixture_body(gsim.cfg)
    for envs in groups:
        idx = torch.as_tensor(list(envs), device=gsim.device)
        want = contacts_ref.contacts_ref(cpu(gsim.ws_cnt[idx]), cpu(gsim.ws_key[idx]), cpu(gsim.ws_acc[idx]), gsim.contact_capacity, N, M, body, k)
        SC.same_contacts([None if t is None else t[idx] for t in got], want, '%s, envs %s' % (what, list(envs)))
    for (name, _, _), t in zip(shapes, [t for t in got if t is not None]):
        no_differences(replica_differences(t[:replicas]), '%s: output %s' % (what, name))
    assert bool((got[0][:D] >= 0).any()), '%s: no contact is listed' % what


@pytest.mark.parametrize('case', OS.STEP_CASES, ids=OS.step_case_id)
def test_step_row(case):
    from gym_kilobots_amd.sim import KilobotSim
    row, allow_sleep = case
    require(OS.step_need(row), row.name)
    t0 = time.time()
    E, N, reps = row.E, row.scene.N, row.E // D
    xy, th, objs = OS.step_start(row)
    osim = OS.step_oracle(row, allow_sleep)
    gsim = KilobotSim(E, N, **OS.step_config_kw(row, allow_sleep))
    gsim.set_poses_m(np.tile(xy, (reps, 1, 1)), np.tile(th, (reps, 1)))
    if objs is not None:
        gsim.set_objects_m(np.tile(objs, (reps, 1, 1)))
    assert nbytes(getattr(gsim, row.tensor)) == E * row.row_bytes and OS.reached(row.row_bytes, E) == row.boundary
    bands = []
    for name in row.banded:         # behind a front band: scratch holds the sentinel, the store its zeros
        t = getattr(gsim, name)
        b = Banded(t.shape, t.dtype, gsim.device, name)
        if name != 'scratch':
            b.view.copy_(t)
        setattr(gsim, name, b.view)
        bands.append(b)
        del t
    gsim._bind()
    torch.cuda.empty_cache()
    probes = OS.probes(row.row_bytes, E)
    fields = ('x', 'y', 'theta') + (('sleep_time',) if allow_sleep else ()) + (OBJ_FIELDS[3:] if objs is not None else ())
    t1 = time.time()
    launches = OS.step_launches(row)
    for k, (n, a) in enumerate(launches):
        what = '%s sleep %d, launch %d' % (row.name, allow_sleep, k)
        osim.set_actions(a)
        osim.step(n, threads=D)
        gsim.step(n, actions=dev(a).repeat(reps, 1, 1))
        torch.cuda.synchronize()
        held_to_the_oracle(osim, gsim, range(D), fields, what)
        held_to_the_oracle(osim, gsim, probes, fields, what + ', probe envs')
        replicas_hold(gsim, what)
        assert int((gsim.status != 0).sum()) == 0 and int(osim.status.max()) == 0, '%s: status is not 0 in %d envs' % (what, int((gsim.status != 0).sum()))
        check_bands(bands, what)
    assert int(gsim.ws_cnt[:D].sum(1, dtype=torch.int64).min()) > 0, 'every distinct env has contacts'
    t2 = time.time()
    tail = range(E - D, E)          # the last D envs: wholly above the boundary, scene 0 .. D - 1 in this order
    if row.masked:
        assert (E - D) * row.row_bytes >= B32 and (E - D) % D == 0
        mask = torch.zeros(E, dtype=U8, device=gsim.device)
        mask[E - D:] = 1
        names = [n for n in GD.bound_fields(gsim) if n != 'scratch']
        snap = {n: getattr(gsim, n)[:E - D].clone() for n in names}
        n, a = launches[-1]
        moved = fields + ('v', 'w')

        def others_unchanged(what):
            for name in names:
                assert torch.equal(GD.bits(getattr(gsim, name)[:E - D]), GD.bits(snap[name])), '%s: field %s of an env that the mask does not select changed' % (what, name)

        what = '%s sleep %d, masked step' % (row.name, allow_sleep)
        osim.set_actions(a)
        osim.step(n, threads=D)
        gsim.step(n, actions=dev(a).repeat(reps, 1, 1), env_mask=mask)
        torch.cuda.synchronize()
        held_to_the_oracle(osim, gsim, tail, moved, what)
        others_unchanged(what)
        check_bands(bands, what)
        what = '%s sleep %d, reset_envs' % (row.name, allow_sleep)
        kw = dict(seed=OS.RESET_SEED, std=OS.RESET_STD, random_theta=True, resolve=True)
        gsim.reset_envs(mask, **kw)
        R.ref_reset_envs(osim, np.ones(D, np.uint8), env_offset=E - D, **kw)
        torch.cuda.synchronize()
        held_to_the_oracle(osim, gsim, tail, moved, what)
        others_unchanged(what)
        assert int((gsim.status != 0).sum()) == 0 and int(osim.status.max()) == 0, what
        check_bands(bands, what)
        del snap
    t3 = time.time()
    what = '%s sleep %d, contacts' % (row.name, allow_sleep)
    groups = [range(D), [p for p in probes if p < E - D]] + ([tail] if row.masked else [[E - 1]])
    contacts_hold(gsim, groups, E - D if row.masked else E, what)
    check_bands(bands, what)
    if row.masked:          # kb_reset of every env: each has a spawn of its own, the last D are the oracle's with this offset
        what = '%s sleep %d, reset' % (row.name, allow_sleep)
        kw = dict(seed=OS.RESET_SEED + 1, std=OS.RESET_STD, random_theta=True)
        gsim.reset(**kw)
        osim.reset(env_offset=E - D, **kw)
        torch.cuda.synchronize()
        held_to_the_oracle(osim, gsim, tail, fields + ('v', 'w'), what)
        check_bands(bands, what)
    gsim.close()
    print('large offsets, %s sleep %d: %d envs, %s %.2f GB, probes %s; allocation %.1f s, %d launches and their comparison %.1f s, masked part %.1f s, contacts and reset %.1f s'
          % (row.name, allow_sleep, E, row.tensor, E * row.row_bytes / 1e9, probes, t1 - t0, len(launches), t2 - t1, t3 - t2, time.time() - t3))
