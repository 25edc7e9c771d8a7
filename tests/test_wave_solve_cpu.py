"""The scenes of tests/wave_solve_scenes.py without a GPU: on the oracle every scene has, in the launches that
tests/test_wave_solve_gpu.py runs, what it is there for, as far as the oracle's outputs show it -- islands on several waves
whose position sweeps take different numbers of iterations (closed form of a pair at rest), kilobots of every kind of
ownership, the three sleep blocks, a candidate of the continuous step next to a many-iteration island, the change of solver
path -- and stays on the register path wherever it claims to.  These are conditions on the scenes, not measurements."""
import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from oracle import oracle as O
from tests import label_scenes as LS
from tests import setup_scenes as SS
from tests import solver_regimes as SR
from tests import toi_scenes as TS
from tests import wave_solve_scenes as WS
from tests.host_common import lib  # noqa: F401

# distances in world units from float32 coordinates of up to 25: a float has steps of 2e-6 there, a distance is a few
# operations on them; two closed forms one iteration apart differ by 0.2 (2 slop) = 2e-3 at least
DIST_TOL, FORM_GAP = 2e-5, 1e-3


def test_closed_form_of_a_pair_at_rest():
    for mm, n in zip(WS.DEEP_MM, (4, 7, 10, 10, 10, 10, 10)):
        sep = (mm * 1e-3 - WS.DIAMETER) * WS.WORLD
        assert WS.pair_iterations(sep) == n, (mm, WS.pair_iterations(sep))
    assert WS.pair_iterations((0.0328 - WS.DIAMETER) * WS.WORLD) == 1
    # an island that needs n iterations: the last one finds it inside 3 slop, the one before does not
    d = 0.0321 * WS.WORLD
    assert WS.pair_after(d, 3) - WS.DIAMETER * WS.WORLD >= -3 * WS.SLOP > WS.pair_after(d, 2) - WS.DIAMETER * WS.WORLD


def _dist(x, y, a, b):
    return float(np.hypot(float(x[a]) - float(x[b]), float(y[a]) - float(y[b])))


@pytest.mark.parametrize('case', WS.cases(), ids=WS.case_id)
def test_scene_has_on_the_oracle_what_it_is_there_for(lib, case):
    s, allow_sleep = case
    nw, capL, cap = SR.bands(lib, nat, s.N, 0, allow_sleep)
    assert nw == {1024: 8, 200: 2, 64: 1}[s.N]
    E = len(s.envs)
    xy, th, st, role, ids = WS.plant(s)
    assert (np.abs(xy[..., 0]) < 0.99).all() and (np.abs(xy[..., 1]) < 0.74).all() and 2 <= E <= 3
    osim = O.OracleSim(O.default_config(E, s.N, allow_sleep=allow_sleep))
    osim.set_poses_m(xy, th)
    if allow_sleep:
        osim.sleep_time[...] = st
    x0, y0 = osim.x.copy(), osim.y.copy()
    on_reg = [[] for _ in range(E)]
    slept = []
    for k in range(WS.SINGLE_LAUNCHES):
        xb, yb = osim.x.copy(), osim.y.copy()
        a = WS.actions(s, k, role)
        assert (a[role == 'move'][:, 0] >= 0.1 * WS.SPEED * WS.FULL).all()
        osim.set_actions(a)
        osim.step(1)
        assert int(osim.status.max()) == 0, (s.name, k, osim.status)
        slept.append(osim.sleep_time.copy() if allow_sleep else None)
        for e in range(E):
            key, cnt = osim.ws_key[e], osim.ws_cnt[e]
            sizes = SS.islands(key, cnt)
            assert 0 < sum(sizes) <= capL, (s.name, e, k, sum(sizes))
            on_reg[e].append(SS.on_register_path(sizes, nw))
            if k == 0:
                _first_launch(s, e, nw, ids[e], role[e], sizes, key, cnt, (xb[e], yb[e]), (osim.x[e], osim.y[e]), allow_sleep)
        print('%s sleep %d launch %d: ' % (s.name, allow_sleep, k) + ' | '.join(
            'contacts %d, largest island %d, register path %s' % (sum(SS.islands(osim.ws_key[e], osim.ws_cnt[e])), SS.islands(osim.ws_key[e], osim.ws_cnt[e])[0],
                                                                  on_reg[e][-1]) for e in range(E)))
    osim.set_actions(WS.actions(s, WS.SINGLE_LAUNCHES, role))
    osim.step(WS.FUSED_SUBSTEPS)
    assert int(osim.status.max()) == 0, (s.name, 'fused', osim.status)
    for e in range(E):
        if 'path change' in s.has and e == 0:
            # the register path, then the cooperative sweep, then the register path again -- beside an env that never leaves it
            r = on_reg[e]
            assert r[0] and not all(r), r
            off = r.index(False)
            assert any(r[off:]), r
        else:
            assert all(on_reg[e]), (s.name, e, on_reg[e])
    if 'sleep' in s.has and allow_sleep:
        for e in range(E):
            for z in ids[e].get('sleepers', []) + ids[e].get('sleepers3', []):
                # asleep beside awake kilobots: never moved
                assert all((sl[e, z] < 0).all() for sl in slept) and (osim.sleep_time[e, z] < 0).all()
                assert np.array_equal(osim.x[e, z], x0[e, z]) and np.array_equal(osim.y[e, z], y0[e, z])
            for z in ids[e]['dozer']:
                # falls asleep inside the fused launch
                assert (slept[-1][e, z] >= 0).all() and (osim.sleep_time[e, z] < 0).all(), (slept[-1][e, z], osim.sleep_time[e, z])
            for z in ids[e]['leaver']:
                # asleep until its neighbour is commanded away
                assert (slept[WS.LEAVE - 1][e, z] < 0).all() and (slept[WS.LEAVE][e, z] >= 0).all()
        awake = (st >= 0)
        assert (slept[0][awake] >= 0).all()


def _first_launch(s, e, nw, where, role, sizes, key, cnt, before, after, allow_sleep):
    """what launch 0 of env e must show"""
    deg, wdeg, owned = WS.degrees(key, cnt)
    pairs = LS.pairs(key, cnt)
    xb, yb = before
    xa, ya = after
    thr = -3.0 * WS.SLOP
    sep = lambda x, y, a, b: _dist(x, y, a, b) - WS.DIAMETER * WS.WORLD      # noqa: E731
    for kind, groups in where.items():
        if kind.startswith('deep') and kind[4:5].isdigit():
            for a, b in groups:
                # a pair at rest: the oracle's centre distance is the n-iteration form, and not the one of n - 1
                d0 = _dist(xb, yb, a, b)
                n = WS.pair_iterations(d0 - WS.DIAMETER * WS.WORLD)
                d1 = _dist(xa, ya, a, b)
                assert n >= 4 and abs(d1 - WS.pair_after(d0, n)) < DIST_TOL, (kind, n, d1, WS.pair_after(d0, n))
                assert abs(d1 - WS.pair_after(d0, n - 1)) > FORM_GAP, (kind, n, d1, WS.pair_after(d0, n - 1))
    if 'out of step' in s.has:
        loads = SS.wave_loads(sizes, nw)
        big = [k_ for k_ in ('mesh3', 'mesh2', 'deephex') if k_ in where][0]
        members = set(int(a) for a in where[big][0])
        inside = [(a, b) for a, b in pairs if a in members and b in members]
        assert len(inside) == sizes[0] and loads[0] >= sizes[0], (len(inside), sizes[:3], loads)
        assert sum(1 for n in loads if n) >= 2, loads                      # the small islands lie on other waves
        seps = [sep(xb, yb, a, b) for a, b in inside]
        small = 'shallow' if big == 'deephex' else None
        if big == 'deephex':
            # the largest island needs several iterations, the small ones a single one
            assert min(seps) < 2 * thr
            assert all(sep(xb, yb, a, b) >= thr and sep(xa, ya, a, b) >= thr for a, b in where[small])
        else:
            # the largest island needs one iteration (it is at rest: nothing deepens it), small ones four to ten
            assert len(inside) >= 40 and min(seps) >= thr and min(sep(xa, ya, a, b) for a, b in inside) >= thr
            assert any(k_.startswith('deep') for k_ in where if k_ != big)
    if 'everybody' in s.has:
        moving = role == 'move'
        lone = moving & (deg == 0) & (wdeg == 0)
        partner_only = moving & (owned == 0) & (deg >= 1)
        wall_only = moving & (deg == 0) & (wdeg == 1)
        corner = moving & (deg == 0) & (wdeg == 2)
        assert lone.any() and partner_only.any() and wall_only.any() and corner.any(), (lone.sum(), partner_only.sum(), wall_only.sum(), corner.sum())
        want = (2, 6) + ((12,) if 'hex12' in where else ())
        assert all((moving & (deg == d)).any() for d in want), np.bincount(deg[moving])
    if 'ram' in s.has and 'ram' in where:
        (r,), = where['ram']
        total, tt = TS.thresholds(TS.DEFAULT_RADIUS)
        step = TS.step_length(TS.DEFAULT_RADIUS)
        d0 = TS.wall_dists(xb[r], yb[r])[0]
        assert d0 > total and not TS.no_event(np.float32(d0), np.float32(d0 - step), tt)     # free for the substep, and it would end inside tt
        assert TS.wall_dists(xa[r], ya[r])[0] > d0 - step + 0.002                               # ... the continuous step held it back
        assert any(k_.startswith('deep') for k_ in where)                                       # beside islands of many iterations


def test_the_scenes_select_the_kernels_they_are_there_for(tmp_path):
    from tests import variant_census as VC
    cases = WS.cases()
    listed, selected = VC.host_census(tmp_path, [SR.plan_inputs(s.N, 0, sl) for s, sl in cases])
    for (s, sl), (status, index) in zip(cases, selected):
        drive, light, obj, fn, tier, poly, sense, sleep = listed[index]
        assert status == 0 and (obj, sleep) == (0, sl) and fn == (1024 if s.N == 1024 else 0), (s.name, listed[index])
