"""What tests/test_large_offsets_gpu.py rests on, without a device (tests/offset_scenes.py): every batch size, straddling
env and probe set follows from the ABI constants; no straddling env of a claimed boundary is a multiple of D; the scenes
keep their regimes and status 0 on the oracle at contact_capacity = 65528, and their five envs and the five restated
outputs of every row differ pairwise; the table leaves out no launching method of KilobotSim; and the host side refuses
or widens where it has to (kb_sense_edges at 2^31 nodes, kb_scratch_bytes as a 64-bit value, the grid products)."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from tests import offset_scenes as OS
from tests import reduce_ref
from tests import residency_scenes as RS
from tests import solver_regimes as SR

D, B31, B32 = OS.D, OS.B31, OS.B32


@pytest.fixture(scope='module')
def lib():
    return nat.load()


def handle(lib, E, N, **kw):
    cfg = nat.default_config(E, N, **kw)
    h = C.c_void_p()
    nat.call(lib, 'kb_create', C.byref(cfg), C.byref(h))
    return h


# ---- the sizes --------------------------------------------------------------------------------------------------------------
def test_the_constants_are_those_of_the_abi(lib):
    assert (OS.MAX_BOTS, OS.MAX_NEIGHBORS, OS.HIST_MAX_BINS, OS.MAX_RAYS, OS.GRID_MAX_SIDE, OS.FIELD_MAX_CHANNELS, OS.RENDER_MAX_SIDE, OS.REDUCE_MAX_CHANNELS,
            OS.MAX_OBJECTS) == (nat.MAX_BOTS, nat.MAX_NEIGHBORS, nat.HIST_MAX_BINS, nat.MAX_RAYS, nat.GRID_MAX_SIDE, nat.FIELD_MAX_CHANNELS, nat.RENDER_MAX_SIDE,
                                nat.REDUCE_MAX_CHANNELS, nat.MAX_OBJECTS)
    assert OS.HIST[0] * OS.HIST[1] == nat.HIST_MAX_BINS
    cfg = nat.default_config(1, 8, contact_capacity=OS.MAX_CAPACITY + 8)
    assert lib.kb_create(C.byref(cfg), C.byref(C.c_void_p())) == nat.KB_EINVAL, 'a capacity above %d is accepted' % OS.MAX_CAPACITY
    for N, capacity, cap in ((200, OS.MAX_CAPACITY, OS.MAX_CAPACITY), (1024, 0, OS.FIXED_1024_CAPACITY), (256, OS.MAX_CAPACITY, OS.MAX_CAPACITY)):
        h = handle(lib, 3, N, contact_capacity=capacity)
        assert lib.kb_contact_capacity(h) == cap
        assert lib.kb_scratch_bytes(h) == 3 * OS.scratch_row_bytes(cap)
        lib.kb_destroy(h)
    assert OS.GRID_CHANNELS == 5 and RS.BOXES['num_objects'] == 2


def check_batch(row_bytes, boundary, E, what):
    s, f = OS.straddler(row_bytes, boundary), OS.first_above(row_bytes, boundary)
    assert s * row_bytes <= boundary < (s + 1) * row_bytes, what
    assert f * row_bytes >= boundary > (f - 1) * row_bytes, what
    assert E % D == 0 and E - f >= D > E - D - f, '%s: %d envs, the first whole env above the boundary is %d' % (what, E, f)
    assert E * row_bytes > boundary
    assert s % D != 0, '%s: env %d straddles the boundary and carries scene 0' % (what, s)
    p = OS.probes(row_bytes, E)
    assert s in p and f in p and E - 1 in p and p == sorted(set(p)) and p[-1] == E - 1, (what, p)
    if boundary == B32:         # the lower boundary is probed as well
        s31 = OS.straddler(row_bytes, B31)
        assert s31 in p and OS.first_above(row_bytes, B31) in p
        # where that env carries scene 0, the boundary is not at the start of its row: bytes wrapped to the front of the tensor
        # land inside env 0's row, shifted, and every replica comparison of env 0 sees them
        assert s31 % D != 0 or B31 % row_bytes != 0, '%s: env %d begins at 2^31 bytes and carries scene 0' % (what, s31)


@pytest.mark.parametrize('row', OS.STEP_ROWS, ids=lambda r: r.name)
def test_step_row_sizes(row, lib):
    check_batch(row.row_bytes, row.boundary, row.E, row.name)
    cap = {'scratch': row.row_bytes // OS.SCRATCH_BYTES_PER_CONTACT, 'ws_key': row.row_bytes // 4}[row.tensor]
    kw = dict(OS.step_config_kw(row, 0))
    h = handle(lib, row.E, row.scene.N, **kw)
    assert lib.kb_contact_capacity(h) == cap
    total = lib.kb_scratch_bytes(h)
    lib.kb_destroy(h)
    assert total == row.E * cap * OS.SCRATCH_BYTES_PER_CONTACT
    assert OS.reached(row.row_bytes, row.E) == row.boundary
    assert OS.step_need(row) > total


def test_the_sizes_the_rows_are_known_by():
    by = OS.STEP_BY_NAME
    r = by['scratch-200-p014']
    assert (r.row_bytes, r.E, OS.probes(r.row_bytes, r.E)) == (2096896, 2055, [1024, 1025, 2048, 2049, 2054])
    assert by['scratch-1024-p022-generic'].E == by['scratch-crowd-mode3'].E == 2055
    r = by['scratch-1024-p022-fixed']
    assert (r.row_bytes, r.E, OS.straddler(r.row_bytes, B31), OS.straddler(r.row_bytes, B32)) == (133120, 32270, 16131, 32263)
    r = by['store-200-p014']
    assert (r.row_bytes, r.E, OS.probes(r.row_bytes, r.E)) == (262112, 8200, [8193, 8194, 8199])
    assert r.E * OS.scratch_row_bytes(OS.MAX_CAPACITY) == 17194547200
    # out of reach: the store at 2^32 bytes
    assert OS.STORE_B32_ENVS == 16395 and OS.STORE_B32_ENVS * OS.scratch_row_bytes(OS.MAX_CAPACITY) > 32 << 30
    assert OS.E_SENSE == 16390 and OS.straddler(256 << 10, B32) == 16384 and OS.straddler(256 << 10, B31) == 8192
    assert OS.E_RENDER == 350 and OS.RENDER_ROW == 12582912
    assert (OS.straddler(OS.RENDER_ROW, B31), OS.straddler(OS.RENDER_ROW, B32)) == (170, 341)
    assert OS.first_crossing_envs(OS.RENDER_ROW, B32) == 342         # kb_render passes 4 GiB at 342 envs
    assert OS.first_crossing_envs(OS.scratch_row_bytes(OS.MAX_CAPACITY), B32) == 2049


@pytest.mark.parametrize('row', OS.CROSSING, ids=lambda r: r.name)
def test_sensing_row_sizes(row):
    sizes = dict(row.outputs)
    check_batch(sizes[row.claims], row.boundary, row.E, row.name)
    run = OS.E_RENDER if row.name == 'render' else OS.E_SENSE          # the handle it runs on
    assert row.E <= run and OS.reached(sizes[row.claims], run) == row.boundary
    assert all(run * b // (b if b % 4 else 4) < B31 for b in sizes.values()), 'element indices stay below 2^31'
    if row.name not in ('render', 'grid'):
        assert sizes[row.claims] == {B32: 256 << 10, B31: 128 << 10}[row.boundary]
    assert OS.sensing_need(row) >= sum(OS.FRONT_BAND + row.E * b for b in sizes.values())


def test_object_points_reaches_no_boundary_with_two_objects():
    sizes = dict(OS.OBJECT_POINTS.outputs)
    assert sizes['obj'] == 32 << 10 and OS.reached(sizes['obj'], OS.E_SENSE) is None
    assert OS._f(OS.N_SENSE * OS.MAX_OBJECTS * 4) == 128 << 10      # with eight objects: the rows of rays


def test_the_entries_that_cannot_cross():
    for name, (method, row_bytes) in OS.CANNOT_CROSS.items():
        assert row_bytes < OS.CANNOT_CROSS_LIMIT, name
        assert OS.first_crossing_envs(row_bytes) > 32768 and OS.reached(row_bytes, OS.E_SENSE) is None, name
    assert OS.first_crossing_envs(OS.CANNOT_CROSS['coverage'][1]) == 32769
    have = {row.name for row in RS.SENSORS}
    assert {n for n in OS.CANNOT_CROSS if n not in ('poses', 'host_state', 'set_actions', 'reset')} <= have


# ---- the table against KilobotSim -------------------------------------------------------------------------------------------
# the public methods of KilobotSim that end in a launch: a new one needs a row in tests/offset_scenes.py and a line here
LAUNCHING_METHODS = ['clusters', 'contacts', 'coverage', 'edges', 'field_step', 'hops', 'host_state', 'light_sense', 'neighbor_histogram', 'neighbor_reduce',
                     'neighbors', 'object_points', 'occupancy_grid', 'paths', 'poses', 'rays', 'render', 'reset', 'reset_envs', 'sense', 'set_actions', 'step',
                     'targets']
LAUNCH = re.compile(r"_call\(\s*'(kb_\w+)'(?![^)]*stream=False)")


def launching_methods():
    """The public methods of KilobotSim whose source hands a stream to a library entry, themselves or through a private method
    (the mechanism of tests/test_sensing_residency_cpu.py, for every entry)."""
    from gym_kilobots_amd.sim import KilobotSim
    source = {name: inspect.getsource(fn) for name, fn in vars(KilobotSim).items() if inspect.isfunction(fn)}
    direct = {name for name, text in source.items() if LAUNCH.search(text)}
    private = {name for name in direct if name.startswith('_')}
    found = {name for name in direct if not name.startswith('_')}
    found |= {name for name, text in source.items() if not name.startswith('_') and any('self.%s(' % p in text for p in private)}
    return sorted(found)


def test_the_table_names_every_launching_method():
    assert launching_methods() == sorted(LAUNCHING_METHODS)
    assert OS.table_methods() == sorted(LAUNCHING_METHODS)
    from tests.test_sensing_residency_cpu import SENSING_METHODS
    assert set(SENSING_METHODS) <= set(LAUNCHING_METHODS)


# ---- the scenes on the oracle -----------------------------------------------------------------------------------------------
def pairwise_distinct(arrays, what):
    for a in arrays:
        a = np.asarray(a)
        assert a.shape[0] == D
        assert len({np.ascontiguousarray(a[e]).tobytes() for e in range(D)}) == D, '%s: two of the %d envs are the same' % (what, D)


@pytest.mark.parametrize('case', OS.STEP_CASES, ids=OS.step_case_id)
def test_step_scene_keeps_its_regimes_at_this_capacity(case, lib):
    row, allow_sleep = case
    o = OS.step_oracle(row, allow_sleep)
    objects = row.scene is OS.CROWD
    band = None if objects else SR.bands(lib, nat, row.scene.N, row.kw['contact_capacity'], allow_sleep)
    seen = []
    for n, a in OS.step_launches(row):
        o.set_actions(a)
        o.step(n, threads=D)
        assert o.status.tolist() == [0] * D
        if not objects:
            seen.append(SR.classify(o.ws_cnt, band))
    if objects:
        assert all(o.count_contacts(e, True)[2] > 3 for e in range(D)), 'every env has kilobots on its objects'
        pairwise_distinct([o.ox, o.oy], row.name)      # (every disc was pushed, each env its own way)
    else:
        SR.check_visits(row.scene, seen, 'capacity %d: ' % band[2])
        assert {'R2', 'R3'} & {r for s in seen for r in s}, 'the global slice of scratch is not used'
    pairwise_distinct([o.x, o.theta, o.ws_cnt], row.name)
    assert (SR.counts(o.ws_cnt) > 0).all()
    if row.masked:      # what follows on the device: one more launch, the reset of the last D envs with its resolve step, the reset of all
        from tests import reset_envs_ref as R
        n, a = OS.step_launches(row)[-1]
        o.set_actions(a)
        o.step(n, threads=D)
        assert o.status.tolist() == [0] * D
        kw = dict(std=OS.RESET_STD, random_theta=True, env_offset=row.E - D)
        R.ref_reset_envs(o, np.ones(D, np.uint8), seed=OS.RESET_SEED, resolve=True, **kw)
        assert o.status.tolist() == [0] * D and (SR.counts(o.ws_cnt) > 0).all(), (o.status, SR.counts(o.ws_cnt))
        pairwise_distinct([o.x, o.ws_cnt], row.name + ' after the reset')
        o.reset(seed=OS.RESET_SEED + 1, **kw)
        assert o.status.tolist() == [0] * D and (SR.counts(o.ws_cnt) > 0).all()


def test_1024_kilobots_at_the_largest_capacity_run_the_generic_kernel(lib):
    """The fixed-size kernel has one capacity, 4160: its slice of scratch is 133 120 bytes whatever the configuration asks for,
    so it has a row of its own at the batch that takes that slice to 2^32 bytes."""
    index = {}
    for key, (N, capacity) in dict(generic200=(200, OS.MAX_CAPACITY), big1024=(1024, OS.MAX_CAPACITY), fixed=(1024, 0)).items():
        h = handle(lib, 1, N, contact_capacity=capacity, allow_sleep=0)
        index[key] = lib.kb_variant_index(h)
        lib.kb_destroy(h)
    assert index['big1024'] == index['generic200'] != index['fixed'], index


@pytest.fixture(scope='module')
def sensing_oracle():
    return OS.sensing_oracle()


def test_why_the_sensing_scene_is_not_stepped():
    """After the first substep of the residency module's run more than 64 kilobots lie on one box in every env: the device
    flags that (status bit 4) and the oracle does not."""
    from tests import contacts_ref
    o = OS.sensing_oracle()
    o.set_actions(RS.spawn(OS.N_SENSE)[3])
    o.step(1, threads=D)
    assert o.status.tolist() == [0] * D
    for e in range(D):
        keys = o.ws_key[e][:int(SR.counts(o.ws_cnt)[e])]
        assert max(int((keys == contacts_ref.KEY_OBJ + f).sum()) for f in range(RS.BOXES['num_objects'])) > OS.OBJ_LIST, e


@pytest.mark.parametrize('name', [r.name for r in OS.CROSSING if r.name != 'render'] + ['object_points'])
def test_the_five_restated_outputs_differ(name, sensing_oracle):
    tab = OS.tables_of(OS.sensing_config(OS.N_SENSE))
    pairwise_distinct(OS.want(name, tab, OS.oracle_state(sensing_oracle)), name)
    if name == 'field_step':
        assert OS.FIELD_MASK.tolist().count(0) == 1
        pairwise_distinct(OS.field_inputs(), 'the inputs of field_step')


def test_the_five_restated_frames_differ():
    o = RS.oracle_run(OS.RENDER_N)
    w = OS.want_render_bands(OS.tables_of(OS.sensing_config(OS.RENDER_N)), OS.oracle_state(o), RS.LIGHTS_M)
    assert w.shape == (D, 192, OS.RENDER_SIDE, 3)
    pairwise_distinct([w], 'render')
    assert not (w == OS.SENTINEL).all(-1).any(), 'a pixel of the frames has the colour of the sentinel'
    assert sorted(set(OS.RENDER_BANDS)) == list(OS.RENDER_BANDS) and OS.RENDER_BANDS[0] == 0 and OS.RENDER_BANDS[-1] == OS.RENDER_SIDE - 1


def degree_sums(o):
    return {R: [int(reduce_ref.in_range(o.x[e], o.y[e], R).sum()) for e in range(D)] for R in OS.EDGE_RADII}


def test_the_edge_list_passes_its_boundaries(sensing_oracle):
    sums = degree_sums(sensing_oracle)
    R, nnz = OS.edges_radius(sums)
    assert R == 0.07 and nnz == 510155140
    assert 16 * nnz > B32 and 4 * nnz > 1 << 30 and nnz < B31
    assert len(set(sums[R])) == D
    per_replica = sum(sums[R])
    at = -(-(B32 // 16) // per_replica) * per_replica       # the first replica that begins above 2^32 bytes of rel
    assert nnz - at >= per_replica, 'a whole replica lies above 2^32 bytes of rel'


# ---- the host side ----------------------------------------------------------------------------------------------------------
def test_edges_refuses_int32_node_ids_that_do_not_exist(lib):
    E = B31 // nat.MAX_BOTS
    offsets = (C.c_int64 * 2)()
    for envs, rc, words in ((E, nat.KB_EINVAL, 'num_envs * num_bots must be below 2^31'), (E - 1, nat.KB_ENOTBOUND, 'kb_bind() first')):
        h = handle(lib, envs, nat.MAX_BOTS)
        got = lib.kb_sense_edges(h, 0.07, C.cast(offsets, C.c_void_p), 0, None, None, None, None, None)
        msg = lib.kb_last_error().decode()
        lib.kb_destroy(h)
        assert got == rc and 'kb_sense_edges' in msg and words in msg, (envs, got, msg)


def test_scratch_bytes_arrive_as_a_64_bit_value(lib):
    row = OS.STEP_BY_NAME['store-200-p014']
    h = handle(lib, row.E, row.scene.N, **OS.step_config_kw(row, 0))
    n = lib.kb_scratch_bytes(h)
    lib.kb_destroy(h)
    assert lib.kb_scratch_bytes.restype is C.c_size_t and C.sizeof(C.c_size_t) == 8
    assert n == 17194547200 and n > B32 and n & 0xFFFFFFFF != n


def grid_products():
    """{launch: workgroups} of the entries whose grid is a product with the env count, restated from kb_abi.hip: tiles of 256
    kilobots or cells (KB_OBJECTS_TILE), bands of GridLds (64 KiB of int32 counters, three words per cell) and of RenderLds."""
    E, N = OS.E_SENSE, OS.N_SENSE
    gw, gh = OS.GRID
    max_rows = (64 << 10) // (4 * 3 * gw)
    cfg = nat.default_config(1, OS.RENDER_N)
    return {'kb_sense_objects': E * -(-N // 256), 'kb_sense_grid, kilobots': E * -(-gh // max_rows), 'kb_sense_grid, objects': E * (gw * gh // 256),
            'kb_field_step': E * OS.FIELD_CHANNELS,
            'kb_render': OS.E_RENDER * nat.render_bands(OS.RENDER_N, cfg.world_width, cfg.world_height, cfg.bot_radius, OS.RENDER_SIDE, OS.RENDER_SIDE)[0],
            'kb_step': max(r.E for r in OS.STEP_ROWS)}


def test_the_grid_products_stay_below_2_31():
    g = grid_products()
    assert g['kb_sense_objects'] == 4 * OS.E_SENSE and g['kb_sense_grid, kilobots'] == 4 * OS.E_SENSE and g['kb_sense_grid, objects'] == 64 * OS.E_SENSE
    assert all(0 < v < B31 for v in g.values()), g
    assert g['kb_render'] >= OS.E_RENDER * (OS.RENDER_SIDE * OS.RENDER_SIDE // 8192), 'a band holds at most 8192 pixels'
