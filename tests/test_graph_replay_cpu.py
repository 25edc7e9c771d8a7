"""What tests/test_graph_replay_gpu.py rests on, without a device (tests/graph_scenes.py): every public method of KilobotSim
that reaches a launch is a row of the table or a written refusal, the step rows cover every translation unit, the inputs of
the replays tell the replays apart on the oracle and the restatements, the edge list of the edges row fits its capacity, and
the refusals say what to do instead."""
import inspect
import re

import numpy as np
import pytest
import torch

from gym_kilobots_amd import _native as nat
from oracle import oracle as O
from tests import assign_ref
from tests import clusters_ref
from tests import edges_ref
from tests import graph_scenes as GS
from tests import hops_ref
from tests import reduce_ref
from tests import reset_envs_ref as R
from tests import residency_scenes as RS
from tests import targets_ref
from tests import variant_census as VC

# the entries of the signature table that launch nothing: no stream, nothing to capture.  Every other entry has to be reached by
# a public method of KilobotSim that is a row or a refusal, or stand under TEST_HOOKS
HOST_ENTRIES = {'kb_create', 'kb_destroy', 'kb_bind', 'kb_histogram_sectors', 'kb_get_outline', 'kb_grid_channels', 'kb_path_costs',
                'kb_render_default_style', 'kb_ray_directions', 'kb_lds_bytes', 'kb_resident_envs_per_cu', 'kb_contact_capacity',
                'kb_lds_staging_entries', 'kb_scratch_bytes', 'kb_light_action_dim', 'kb_light_count', 'kb_block_threads', 'kb_variant_index',
                'kb_set_block_threads', 'kb_exact_division', 'kb_last_error', 'kb_version'}
# launches that KilobotSim does not bind: self-tests of the build that no training loop calls
TEST_HOOKS = {'kb_exact_selftest', 'kb_debug_lds'}


# ---- completeness ---------------------------------------------------------------------------------------------------------
def launches_of_methods():
    """{public method of KilobotSim: the entries it launches on the stream, itself or through a private method}"""
    from gym_kilobots_amd.sim import KilobotSim
    source = {name: inspect.getsource(fn) for name, fn in vars(KilobotSim).items() if inspect.isfunction(fn)}
    direct = {name: {m.group(1) for m in re.finditer(r"_call\(\s*'(kb_\w+)'([^\n]*)", text) if 'stream=False' not in m.group(2)} for name, text in source.items()}
    found = {}
    for name, text in source.items():
        if name.startswith('_'):
            continue
        entries = set(direct[name])
        for other, theirs in direct.items():
            if other != name and theirs and re.search(r'self\.%s\(' % re.escape(other), text):
                entries |= theirs
        if entries:
            found[name] = entries
    return found


def classified():
    """{method: where it stands}, and a method stands in one place only"""
    rows = {row.method: 'SENSING' for row in GS.SENSING}
    places = [rows, GS.STEP_METHODS, dict.fromkeys(GS.REFUSED, 'REFUSED')]
    names = [n for p in places for n in p]
    assert len(names) == len(set(names)), 'a method stands in two places'
    return {n: where for p in places for n, where in p.items()}


def completeness_errors(found, table, entries):
    errors = ['%s launches %s and is neither a row nor a refusal' % (m, sorted(e)) for m, e in sorted(found.items()) if m not in table]
    errors += ['%s stands in the table and launches nothing' % m for m in sorted(table) if m not in found and table[m] != 'REFUSED']      # (a refusal may read the device through torch alone)
    reached = set().union(*found.values()) if found else set()
    errors += ['entry %s is launched by no public method of KilobotSim' % e for e in sorted(entries - HOST_ENTRIES - TEST_HOOKS - reached)]
    return errors


def test_every_launching_method_is_a_row_or_a_refusal():
    found = launches_of_methods()
    assert not completeness_errors(found, classified(), set(nat.SIGNATURES))
    assert HOST_ENTRIES | TEST_HOOKS <= set(nat.SIGNATURES) and not (HOST_ENTRIES | TEST_HOOKS) & set().union(*found.values())
    assert found['edges'] == {'kb_sense', 'kb_sense_edges'} and found['targets'] == {'kb_sense_targets', 'kb_sense_assign'}
    assert {'sense', 'assign', 'paths-128', 'edges'} <= set(GS.SENSING_BY_NAME)
    assert [row.name for row in GS.SENSING] == [row.name for row in RS.SENSORS] + [RS.PATHS_BIG.name]
    assert set(GS.SENSING_INPUTS) <= set(GS.SENSING_BY_NAME) and set(GS.REFUSED_FORMS) <= {row.method for row in GS.SENSING}


def test_the_completeness_check_misses_no_deleted_row_and_no_deleted_refusal():
    found, table = launches_of_methods(), classified()
    for gone in ('paths', 'step', 'host_state'):
        assert any(gone in e for e in completeness_errors(found, {m: w for m, w in table.items() if m != gone}, set(nat.SIGNATURES))), gone
    assert any('kb_new' in e for e in completeness_errors(found, table, set(nat.SIGNATURES) | {'kb_new'}))


def test_the_env_refusals_exist():
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    for name in GS.REFUSED_ENV:
        text = inspect.getsource(getattr(BatchedKilobotsEnv, name))
        assert 'refuse_capture' in text or 'self._path_mask(' in text, name         # (_path_mask refuses for whoever hands it cells)
    assert 'refuse_capture' in inspect.getsource(BatchedKilobotsEnv._path_mask)
    from gym_kilobots_amd.sim import KilobotSim
    for name in list(GS.REFUSED) + list(GS.REFUSED_FORMS):
        assert 'refuse_capture' in inspect.getsource(getattr(KilobotSim, name)), name


# ---- the step rows --------------------------------------------------------------------------------------------------------
def test_one_step_row_per_translation_unit():
    assert sorted(GS.STEP_UNITS) == GS.units_in_tree() and len(GS.STEP_UNITS) == 12
    scenes = {}
    for unit in GS.STEP_UNITS:
        row = GS.step_row(unit)
        assert GS.unit_of(row[2]) == unit, (unit, row)
        scenes[unit] = VC.scene(row)
        assert scenes[unit].E <= 8
    variant = {unit: GS.step_row(unit)[2] for unit in GS.STEP_UNITS}       # (drive, light, obj, fn, tier, poly, sense, sleep)
    assert variant[GS.FIXED][3] == 1024 and scenes[GS.FIXED].E == 2 and scenes[GS.FIXED].N == 1024
    assert any(v[7] and scenes[u].kw['allow_sleep'] == 1 for u, v in variant.items())
    assert any(v[2] and not v[5] for v in variant.values()) and any(v[2] and v[5] for v in variant.values())      # discs, polygons
    assert any(s.mode in (O.DRIVE_SIMPLE_PHOTOTAXIS, O.DRIVE_PHOTOTAXIS) and s.light == O.LIGHT_MOMENTUM and GS.light_action_dim(s) == 2 for s in scenes.values())
    assert any(s.mode == O.DRIVE_MIXED for s in scenes.values())
    assert len(GS.MASKS) == GS.REPLAYS and all(len(m) == VC.E for m in GS.MASKS) and [0, 1] in [sorted(m) for m in GS.MASKS]


@pytest.mark.parametrize('unit', list(GS.STEP_UNITS))
def test_every_step_replay_moves_every_env_it_selects(unit):
    s = VC.scene(GS.step_row(unit))
    for form in GS.FORMS:
        osim = VC.oracle_sim(s)
        for k in range(GS.REPLAYS):
            was = {f: getattr(osim, f).copy() for f in GS.STEP_OUTPUTS}
            if form == 'fused' and k > 0:
                a, la, _ = GS.step_inputs(s, k)
                if a is not None:
                    osim.set_actions(a)
                osim.step(1, light_action=la)
            GS.oracle_form(osim, s, form, k)
            sel = np.array(GS.MASKS[k] if form == 'masked' else [1] * s.E, bool)
            for f in GS.STEP_OUTPUTS:
                moved = (getattr(osim, f) != was[f]).any(1)
                assert moved[sel].all() and not moved[~sel].any(), (unit, form, k, f)
        assert int(osim.status.max()) == 0, (unit, form)
    for k in range(1, GS.REPLAYS):
        for now, last in zip(GS.step_inputs(s, k), GS.step_inputs(s, k - 1)):
            assert now is None or not np.array_equal(now, last)


# ---- the sensing rows -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def poses():
    """(x, y, theta) of the sensing scene at every replay"""
    return [(o.x.copy(), o.y.copy(), o.theta.copy()) for o in GS.sensing_oracle(RS.N)]


def test_the_edge_list_fits_its_capacity(poses):
    nnz = [int(edges_ref.restate(x, y, th, RS.RADIUS)[4][-1]) for x, y, th in poses]
    assert tuple(nnz) == GS.EDGES_NNZ and max(nnz) <= GS.EDGES_CAPACITY < 2 * min(nnz)
    assert len(set(nnz)) == GS.REPLAYS


def test_the_inputs_of_the_replays_differ():
    for n in (RS.N, RS.N_PATHS):
        base = RS.inputs(n)
        seen = [base] + [GS.sensing_inputs(n, k) for k in range(GS.REPLAYS)]
        for name in base:
            for i in range(len(seen)):
                for j in range(i + 1, len(seen)):
                    assert not np.array_equal(seen[i][name], seen[j][name]), (name, i, j)
                    assert seen[i][name].shape == seen[j][name].shape and seen[i][name].dtype == seen[j][name].dtype
    used = {name for names in GS.SENSING_INPUTS.values() for name in names}
    assert used == set(RS.inputs()), 'an input of the scene that no row reads, or a row that reads none of them'
    for k in range(1, GS.REPLAYS):
        assert not np.array_equal(GS.between_actions(RS.N, k), GS.between_actions(RS.N, k - 1))


def restated(name, x, y, th, v):
    """The outputs of a row whose restatement needs no more than the poses and the inputs, as a dict."""
    if name == 'sense':
        return dict(count=np.stack([reduce_ref.in_range(x[e], y[e], RS.RADIUS).sum(1) for e in range(GS.D)]))
    if name == 'edges':
        return dict(zip(('src', 'dst', 'rel', 'count', 'offsets'), edges_ref.restate(x, y, th, RS.RADIUS)))
    if name == 'hops':
        return dict(zip(('hops', 'parent', 'root', 'stats'), hops_ref.restate(x, y, v['seeds'], RS.RADIUS)))
    if name == 'clusters':
        return dict(zip(('label', 'size', 'table', 'stats'), clusters_ref.restate(x, y, RS.RADIUS)))
    if name == 'targets':
        return targets_ref.restate(x, y, th, v['points'], RS.TARGET_TOL)._asdict()
    if name == 'assign':
        return assign_ref.restate(x, y, th, v['points'], RS.TARGET_TOL, RS.ASSIGN_CUTOFF)._asdict()
    raise KeyError(name)


@pytest.mark.parametrize('name', ['sense', 'edges', 'hops', 'clusters', 'targets', 'assign'])
def test_every_output_differs_from_one_replay_to_the_next(name, poses):
    """The rows whose outputs are integers of the poses: counts, node ids, labels, hop counts, owners.  (The float outputs of
    every row move with the poses; the device test asserts the condition for every output of every row on its eager side.)"""
    row = GS.SENSING_BY_NAME[name]
    before = None
    for k, (x, y, th) in enumerate(poses):
        now = restated(name, x, y, th, GS.sensing_inputs(RS.N, k))
        assert set(row.outputs) - {'nnz'} <= set(now), (set(row.outputs), set(now))
        if before is not None:
            for out in row.outputs:
                if out not in row.few and out != 'nnz':
                    a, b = np.asarray(now[out]), np.asarray(before[out])
                    assert a.shape != b.shape or not np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), (name, out, k)
        before = now


def test_the_assign_row_tells_the_distinct_envs_apart():
    """The row that tests/test_sensing_residency_gpu.py gets with this table: its outputs differ between the five envs, and the
    cutoff leaves slots unmatched."""
    o = RS.oracle_run()
    got = assign_ref.restate(o.x, o.y, o.theta, RS.inputs()['points'], RS.TARGET_TOL, RS.ASSIGN_CUTOFF)
    for part in got:
        assert len({np.ascontiguousarray(part[e]).tobytes() for e in range(RS.D)}) == RS.D
    assert (got.owner == -1).any() and (got.owner >= 0).any() and (got.index == -1).any()


# ---- the reset rows -------------------------------------------------------------------------------------------------------
def test_the_reset_rows_select_and_move():
    c = R.CASES[GS.RESET_CASE]
    assert len(GS.RESET_MASKS) == GS.REPLAYS and all(len(m) == c['E'] for m in GS.RESET_MASKS)
    for k in range(GS.REPLAYS):
        mask, objects, lights = GS.reset_inputs(k)
        assert 0 < mask.sum() < c['E'] and objects.dtype == lights.dtype == np.float32
        if k:
            last = GS.reset_inputs(k - 1)
            assert (mask & last[0]).any(), 'no env is selected in two replays running'
            assert not np.array_equal(objects, last[1]) and not np.array_equal(lights, last[2]) and not np.array_equal(mask, last[0])
    # the spawn of an env follows its counter word
    cfg = R.make_oracle(GS.RESET_CASE).cfg
    kw = {k: v for k, v in R.reset_kw(GS.RESET_CASE).items() if k != 'resolve'}
    kw['seed'] = GS.RESET_SEED
    counters = np.cumsum(GS.RESET_MASKS, 0)
    draws = [R.spawn(cfg, z=z, **kw) for z in counters]
    for k in range(1, GS.REPLAYS):
        both = np.array(GS.RESET_MASKS[k], bool) & np.array(GS.RESET_MASKS[k - 1], bool)
        for now, last in zip(draws[k][:3], draws[k - 1][:3]):
            assert (now[both] != last[both]).any(1).all()


# ---- the env row ----------------------------------------------------------------------------------------------------------
def test_the_env_row_resets_at_steps_three_and_six():
    """The episodes of the env row on the oracle backend, without the observations (they do not act on the state): an env
    reaches its third step at steps 3 and 6 and gets another spawn each time, and done_fn ends episodes early."""
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    kw = GS.env_kw()
    state_kw = {k: kw[k] for k in list(RS.BOXES) + ['allow_sleep', 'spawn_std', 'seed', 'on_status', 'auto_reset', 'max_episode_steps', 'object_init']}
    assert kw['on_status'] == 'ignore' and kw['auto_reset'] and kw['max_episode_steps'] == GS.ENV_EPISODE
    env = BatchedKilobotsEnv(GS.ENV_E, GS.ENV_N, sim_factory=R.MaskedOracleBackend, reward_fn=GS.env_reward, done_fn=GS.env_done, **state_kw)
    env.reset()
    at, early = {}, 0
    for k in range(GS.ENV_REPLAYS):
        obs, reward, done, info = env.step(torch.from_numpy(GS.env_actions(k)))
        timed_out = done & (info['episode_length'] == GS.ENV_EPISODE)
        early += int((done & ~timed_out).sum())
        at[k + 1] = (timed_out.clone(), obs.clone())
        assert float(reward.min()) > 0.0 and int(env.sim.status.max()) == 0
    both = at[GS.ENV_EPISODE][0] & at[2 * GS.ENV_EPISODE][0]
    assert bool(both.any()) and early > 0
    assert bool((at[GS.ENV_EPISODE][1][both] != at[2 * GS.ENV_EPISODE][1][both]).flatten(1).any(1).all())
    # every observation option of the env that runs on the device is switched on
    from gym_kilobots_amd.envs.batched_env import OPTIONS
    assert all(kw.get(name) is not None for name in OPTIONS), [name for name in OPTIONS if kw.get(name) is None]


# ---- the refusals ---------------------------------------------------------------------------------------------------------
def test_nothing_is_refused_outside_a_capture_or_without_a_device():
    assert nat.capturing() is False
    nat.refuse_capture('anything', 'nothing')


def test_the_refusals_name_the_way_out(monkeypatch):
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    from gym_kilobots_amd.sim import KilobotSim
    from tests.oracle_backend import OracleBackend
    points = np.zeros((4, 2), np.float32)
    env = BatchedKilobotsEnv(2, 8, sim_factory=OracleBackend, on_status='raise', target_obs=(points, 0.01), path_obs=(8, 6))
    env.reset()
    sim = KilobotSim.__new__(KilobotSim)        # no handle and no device: a refusal comes before either is touched
    sim.num_envs, sim.num_bots, sim._h = 2, 8, None
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    cells = np.zeros((6, 8), np.uint8)
    cases = {
        'edges(capacity=None)': (lambda: sim.edges(0.07), 'capacity=int'),
        'status_bits()': (lambda: sim.status_bits(), 'outside the capture'),
        "check_status('warn')": (lambda: sim.check_status('warn'), "mode='ignore'"),
        'host_state()': (lambda: sim.host_state(), 'outside the capture'),
        'path_cells()': (lambda: sim.path_cells(torch.zeros(1, 2), 8, 6), 'before the capture'),
        "step() with on_status='raise'": (lambda: env.step(None), "on_status='ignore'"),
        "reset() with on_status='raise'": (lambda: env._check_status('reset()'), "on_status='ignore'"),
        'set_targets(points_m)': (lambda: env.set_targets(points_m=points), 'before the capture'),
        'set_path_goal()': (lambda: env.set_path_goal(points_m=points), 'before the capture'),
        'set_path_blocked()': (lambda: env.set_path_blocked(cells), 'before the capture'),
    }
    for what, (call, way_out) in cases.items():
        with pytest.raises(ValueError) as err:
            call()
        msg = str(err.value)
        assert msg.startswith(what) and 'cannot be captured in a graph' in msg and way_out in msg, msg
    with pytest.raises(ValueError, match='cannot be captured'):
        env.set_path_goal(cells=cells)
    # what reads nothing is not refused
    assert sim.check_status('ignore') == 0
    env.set_targets(slot_select=None)
    env.set_path_blocked(None)
    env._on_status = 'ignore'
    env._check_status('step()')
