"""The limits model and the boundary scenes without a GPU (tests/limits_model.py, tests/limit_scenes.py, tests/fuzz_scenes.py):

  * the model counts what independent geometry counts;
  * every row's AT scene sits at exactly its limit and its OVER scene one past it, with every other modelled quantity below
    its limit and the oracle's own flags (status bits 0 and 1) clear -- in the three-env launches the device test runs;
  * kb_create selects the kernel, staging size and wave count the row names;
  * the partner limit cannot be met alone (the proof in tests/limits_model.py, held on piles);
  * stepping the oracle substep by substep, as the fuzz sweep now does, equals the fused call bit for bit;
  * of the default seeds of the fuzz sweep at least 30 scenes are compared through all twelve launches."""
import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from oracle import oracle as O
from tests import fuzz_scenes as FS
from tests import limit_scenes as LS
from tests import limits_model as LM
from tests import solver_regimes as SR
from tests import variant_census as VC
from tests.host_common import lib  # noqa: F401


# ---- the model against plain geometry -----------------------------------------------------------------------------------
def _brute_force(cfg, x, y):
    """(partners [N, 5], {(direction, owner cell): contacts}) from all pairs: b2CollideCircles in float32, the owner of a pair is
    the kilobot that sees the other in its own cell (then the lower id) or to the E, N, NE, NW"""
    N = len(x)
    cx, cy, gw = LM.cells(cfg, x, y)
    rr = np.float32(cfg.bot_radius) * np.float32(25.0)
    rr = rr + rr
    rr2 = rr * rr
    partners, groups = np.zeros((N, 5), np.int64), {}
    k_of = {(0, 0): 0, (1, 0): 1, (0, 1): 2, (1, 1): 3, (-1, 1): 4}
    for a in range(N):
        dx, dy = x - x[a], y - y[a]
        for b in np.flatnonzero(~(dx * dx + dy * dy > rr2)):
            d = (int(cx[b] - cx[a]), int(cy[b] - cy[a]))
            if d not in k_of or (d == (0, 0) and b <= a):
                continue
            partners[a, k_of[d]] += 1
            g = (k_of[d], int(cy[a]) * gw + int(cx[a]))
            groups[g] = groups.get(g, 0) + 1
    return partners, groups


@pytest.mark.parametrize('arena', [(2.0, 1.5), (0.6, 0.6)], ids=['2x1.5', '0.6x0.6'])
def test_model_counts_what_plain_geometry_counts(arena):
    E, N = 2, 200
    rng = np.random.RandomState(5)
    xy = rng.normal(scale=0.05, size=(E, N, 2))
    osim = O.OracleSim(O.default_config(E, N, world_width=arena[0], world_height=arena[1], allow_sleep=0, contact_capacity=8192, ws_slots=64))
    osim.set_poses_m(xy, rng.uniform(-np.pi, np.pi, (E, N)))
    before = (osim.x.copy(), osim.ws_cnt.copy())
    qs = LM.evaluate(osim)
    assert np.array_equal(before[0], osim.x) and np.array_equal(before[1], osim.ws_cnt), 'evaluate must not step the sim it is given'
    for e, q in enumerate(qs):
        partners, groups = _brute_force(osim.cfg, osim.x[e], osim.y[e])
        assert partners.sum() > 2000 and partners.max() >= 10          # (a scene that has something to count)
        assert np.array_equal(q.partners, partners)
        mine = {}
        for (cls, grp), n in q.groups.items():
            key = (LM.DIR_OF_CLASS[cls], grp)
            assert key not in mine, 'the two parities of a direction never share an owner cell'
            mine[key] = n
        assert mine == groups
        assert q.max_rank == max(groups.values()) - 1 and not q.hidden


def test_model_candidates_are_the_kilobots_the_continuous_step_changes():
    """one env of runners and bystanders: with toi_walls on, the oracle moves exactly the model's candidates differently
    from toi_walls off (every runner here has an event; no_event being exact is tests/test_toi_filter_cpu.py)"""
    row = LS.by_name('candidates-bins-256')
    xy, heading = LS.wall_runners(150, LS.WALL_PITCH)
    s = LS.build(row, xy, heading, np.array([LS.TS.FULL, 0.0], np.float32))
    on, off = LS.oracle_sim(row, s), LS.oracle_sim(row, s, toi_walls=0)
    q = LM.evaluate(on)[0]
    on.step(1)
    off.step(1)
    moved = np.flatnonzero((on.x[0] != off.x[0]) | (on.y[0] != off.y[0]))
    assert q.candidates == 150 and np.array_equal(np.sort(s.ids), q.candidate_ids) and np.array_equal(moved, q.candidate_ids)
    assert LM.evaluate(off)[0].candidates == 0          # (without the continuous step nobody is collected)


def test_limits_follow_the_header():
    lim = LM.limits(128, 352, 128, plain=True)
    assert (lim.partners, lim.rank, lim.fixture, lim.depth, lim.candidates) == (63, 255, 64, 86, 128)
    assert LM.limits(1024, 688, 512, plain=True).candidates == 688 and LM.limits(1024, 688, 512, plain=True).depth == 350
    assert LM.limits(256, 200, 256, plain=True).candidates == 200
    assert LM.limits(128, 72, 64, plain=False).candidates == 36 and LM.limits(128, 72, 64, plain=False).depth is None
    assert LM.limits(64, 128, 64, plain=True).depth is None        # one wave: the list sweep, no level table


def test_sweep_decision():
    lim, shape = LM.limits(128, 352, 128, plain=True), LS.SimpleNamespace(threads=128, staging=352, capacity=4096)
    q = lambda ncon, island, asleep=0: LS.SimpleNamespace(ncon=ncon, max_island=island, asleep=asleep)      # noqa: E731
    assert LM.level_sweep(q(128, 100), lim, shape, 0) is False and LM.level_sweep(q(200, 100), lim, shape, 0) is None
    assert LM.level_sweep(q(257, 100), lim, shape, 0) is True and LM.level_sweep(q(353, 20), lim, shape, 0) is True
    assert LM.level_sweep(q(400, 100), lim, shape, 1) is False and LM.level_sweep(q(400, 257), lim, shape, 1) is True
    assert LM.level_sweep(q(10, 5), lim, shape, 2) is True and LM.level_sweep(q(10, 5, asleep=1), lim, shape, 2) is None
    assert LM.level_sweep(q(400, 300), LM.limits(128, 432, 64, plain=False), shape, 0) is False


# ---- the rows -----------------------------------------------------------------------------------------------------------
def test_every_flag_site_has_its_rows():
    """the six sites of status bit 2 and the one of bit 3; the two direction counters (:656, :982) have OVER rows only, and the
    row of a one-wave workgroup at depth 62 does not exist: a one-wave workgroup never runs the level sweep"""
    sites = {}
    for r in LS.ROWS:
        for site in r.sites.split():
            sites.setdefault(site, set()).update(r.whiches)
    assert sites == {':656': {'over'}, ':982': {'over'}, ':834': {'at', 'over'}, ':873': {'at', 'over'}, ':1158': {'at', 'over'},
                     ':1015': {'at', 'over'}, 'kb_coopsolve_bins.inc:62': {'at', 'over'}, ':2557': {'at', 'over'}}
    assert {r.kernel for r in LS.ROWS if r.limit == 'rank'} == {'hashed', 'direct', 'fixed1024', 'objects', 'mixed'}
    assert {r.kernel for r in LS.ROWS if r.limit == 'candidates'} == {'hashed', 'fixed1024', 'objects', 'mixed'}


@pytest.mark.parametrize('row', LS.ROWS, ids=lambda r: r.name)
def test_kb_create_selects_the_kernel_the_row_names(lib, row):
    lim, shape = LS.row_limits(row.name)
    hashed, fixed, threads = LS.expected_shape(row)
    drive, light, obj, fn, tier, poly, sense, sleep = {index: v for _, index, v in VC.rows()}[shape.variant]
    assert shape.threads == threads
    assert (fn == 1024) == fixed and sleep == 0
    assert obj == (row.kernel in ('objects', 'mixed')) and (drive == O.DRIVE_MIXED) == (row.kernel == 'mixed')
    if row.kernel == 'objects':
        assert poly == ('obj_shape' in row.kw) and tier == 1        # the one-wave instantiation, with or without the polygon code
    if row.limit == 'candidates':
        # the small contact_capacity of the issue's rows is what shrinks the staging area below num_bots
        want = {'candidates-bins-256': (200, 200), 'candidates-objects-128': (72, 36), 'candidates-mixed-128': (88, 44),
                'candidates-fixed1024': (688, 688)}[row.name]
        assert (shape.staging, lim.candidates) == want and lim.candidates < row.N
    if row.limit == 'depth':
        assert lim.depth == 86 and shape.threads == 128


@pytest.mark.parametrize('case', LS.cases(), ids=LS.case_id)
def test_row_sits_where_it_claims(lib, case):
    row, which, slot = case
    lim, shape = LS.row_limits(row.name)
    s = LS.scene(row, which, slot)
    osim = LS.oracle_sim(row, s)
    assert osim.cap == shape.capacity
    qs = LM.evaluate(osim)
    osim.step(1)
    assert int((osim.status & 3).max()) == 0, 'contact capacity or warm-start slots ran out: status %s' % osim.status
    for e, q in enumerate(qs):
        sweep = LM.level_sweep(q, lim, shape, row.kw['solver_mode'])
        over = LM.exceeded(q, lim, sweep)
        if e != slot:
            assert over == set() and q.ncon == 0 and q.candidates == 0, (e, over)
            continue
        got = {'rank': q.max_rank, 'fixture': q.max_fixture, 'candidates': q.candidates, 'depth': q.depth, 'partners': q.max_partners}
        want = getattr(lim, row.limit) + (which == 'over')
        assert got[row.limit] == want, (row.name, which, got)
        if row.limit == 'partners':
            # the row that cannot be alone: the partner cell's own group is past the rank limit as well
            assert {'partners', 'rank'} <= over and got['rank'] > 3 * 210
        else:
            assert over == ({row.limit} if which == 'over' else set()), (row.name, which, over, got)
        assert LM.expected_bits(over) == (row.bit if which == 'over' else 0)
        # ... and nothing else is near: every other quantity keeps below its limit
        if row.limit != 'partners':
            for name in ('rank', 'fixture', 'candidates', 'partners', 'depth'):
                if name != row.limit and getattr(lim, name) is not None and got[name] is not None:
                    assert got[name] < getattr(lim, name), (name, got)
        if row.name.endswith('-lds') and row.limit == 'rank':
            assert q.ncon <= shape.staging, 'the pile must fit the LDS staging area, or the row takes the label pass of the global slice'
        if row.limit == 'depth':
            # the cooperative sweep must run, by the contact count alone
            assert sweep is True and SR.regime(q.ncon, shape.threads // 64, shape.staging, shape.capacity) in ('R1', 'R2', 'R3')
        if row.name in LS.NON_INTERACTING:
            assert q.ncon == 0


def test_at_and_over_differ_by_one_kilobot():
    for row in LS.ROWS:
        if row.whiches != ('at', 'over'):
            continue
        lv = getattr(LS.row_limits(row.name)[0], row.limit)
        at, over = LS.planted(row.name, 'at', lv)[0], LS.planted(row.name, 'over', lv)[0]
        assert len(over) == len(at) + 1, row.name
        if row.limit != 'fixture':      # (the ring closes up by one; every other pile keeps its kilobots where they are)
            assert np.array_equal(over[:len(at)], at), row.name


@pytest.mark.parametrize('direction', ['east', 'same'])
def test_63_partners_in_one_direction_never_come_alone(direction):
    """tests/limits_model.py: the partners of one direction lie in one cell within reach of one kilobot, so most of them
    touch each other -- on piles from tight to as loose as reach allows, 63 partners always bring a group past rank 255"""
    assert 3 * (21 * 20 // 2) > LM.RANK + 1 and 63 + 3 * (11 * 10 // 2) + 3 * (10 * 9 // 2) > LM.RANK + 1
    row = LS.by_name('partners-hashed-lds')
    rng = np.random.RandomState(11)
    for reach in (0.004, 0.012, 0.02, 0.0329):
        if direction == 'east':
            # the owner just west of the boundary; partners anywhere in the half disc of `reach` around it, east of the boundary
            owner = np.array([LS.XB - 0.00001, LS.Y0])
            phi, r = rng.uniform(-np.pi / 2, np.pi / 2, 63), reach * np.sqrt(rng.uniform(0.0, 1.0, 63))
            pts = owner + np.stack([0.00002 + r * np.cos(phi), np.clip(r * np.sin(phi), -0.017, 0.017)], -1)
        else:
            owner = LS.CS.cell_centre(LS.CX, LS.CY)
            phi, r = rng.uniform(-np.pi, np.pi, 63), min(reach, 0.017) * np.sqrt(rng.uniform(0.0, 1.0, 63))
            pts = owner + np.stack([r * np.cos(phi), r * np.sin(phi)], -1)
        s = LS.build(row, np.concatenate([owner[None], pts]))
        s.xy[0, s.ids[0]], s.xy[0, 0] = s.xy[0, 0].copy(), s.xy[0, s.ids[0]].copy()      # the owner takes id 0: it owns its same-cell pairs
        q = LM.evaluate(LS.oracle_sim(row, s, contact_capacity=8192))[0]
        assert q.max_partners == 63 and q.max_rank > LM.RANK, (direction, reach, q.max_partners, q.max_rank)


# ---- the fuzz sweep on the oracle and the model ----------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [4, 9, 18, 20, 25, 31])
def test_substep_by_substep_equals_the_fused_call(seed):
    """(scenes with lights, objects, sleeping, mixed laws; launches of 3 and 10 substeps)"""
    s = FS.scene(seed)
    fused, single = FS.oracle_sim(s), FS.oracle_sim(s)
    FS.start(s, fused)
    FS.start(s, single)
    assert any(n > 1 for n, _, _ in s.launches)
    for n_sub, a, la in s.launches:
        for o in (fused, single):
            if a is not None:
                o.set_actions(a)
        fused.step(n_sub, light_action=la)
        for _ in range(n_sub):
            single.step(1, light_action=la)
        for name, _ in O.State._fields_:
            u, v = getattr(fused, name, None), getattr(single, name, None)
            if u is not None and u.size:
                assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), (seed, name)


def test_enough_fuzz_scenes_run_to_the_end(lib):
    """On a device that flags exactly what the model asks for, a scene of the sweep ends early at the capacity flag or at a
    limit; at least 30 of the default seeds must be compared through all twelve launches."""
    ends = {}
    for seed in range(FS.DEFAULT_SEEDS):
        s = FS.scene(seed)
        lim, shape = FS.handle_limits(s, lib, nat)
        launches, why = FS.walk(s, lim, shape)
        ends.setdefault(why, []).append(seed)
        assert (launches == FS.LAUNCHES) == (why is None)
    assert len(ends.get(None, ())) >= 30, ends
