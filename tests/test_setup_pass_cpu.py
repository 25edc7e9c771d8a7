"""The scenes of tests/setup_scenes.py without a GPU: on the oracle every scene has, in the launches that
tests/test_setup_pass_gpu.py runs, what it is there for -- its band of contacts, waves that deal or do not, the exact
contacts per wave, a body with twelve contacts, a rank group of four and more, wall and corner contacts, the two special
pairs, the sleepers -- and stays on the register path (no giant island, no wave above 128 contacts by the placement rule
restated in setup_scenes.py).  These are conditions on the scenes, not measurements."""
import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from oracle import oracle as O
from tests import label_scenes as LS
from tests import setup_scenes as SS
from tests import solver_regimes as SR
from tests.host_common import lib  # noqa: F401


def test_the_planted_structures_are_what_the_docstring_says():
    h = LS.hexagon(SS.CLUSTER_RINGS) * SS.SPACING
    d = np.linalg.norm(h[:, None] - h[None], axis=-1)
    near = (d < 0.033) & ~np.eye(len(h), dtype=bool)
    assert len(h) == 19 and near[0].sum() == SS.DEEP and near.sum() // 2 <= SS.WAVE_CONTACTS
    b = SS.structure('block')
    d = np.linalg.norm(b[:, None] - b[None], axis=-1)
    assert ((d < 0.033) & ~np.eye(len(b), dtype=bool)).sum() // 2 == 128
    s4 = SS.structure('sleepers')
    d = np.linalg.norm(s4[:, None] - s4[None], axis=-1)
    assert ((d < 0.033) & ~np.eye(len(s4), dtype=bool)).sum() // 2 == 24
    # the two special pairs in the numbers the kernel sees: float32 world units
    n = (SS.normals_xy() * SS.WORLD).astype(np.float32)
    assert (n[0] == n[1]).all()
    dd = np.float32(n[3, 0] - n[2, 0]) ** 2 + np.float32(n[3, 1] - n[2, 1]) ** 2
    assert np.float32(1.19209290e-07) ** 2 < dd < 2.0 ** -40, dd        # a contact with a normal of its own, outside kb_exact_guard
    assert SS.wave_loads([1] * 512, 8) == [64] * 8 and SS.wave_loads([2] * 20 + [1] * 480, 8) == [65] * 8
    assert SS.wave_loads([128] + [1] * 440, 8) == SS.WAVE_COUNTS_FIRST[2]
    for s in SS.SCENES:
        xy, th, st, ids = SS.plant(s)
        assert (np.abs(xy[..., 0]) < 0.99).all() and (np.abs(xy[..., 1]) < 0.74).all()
        assert 2 <= len(s.envs) <= 4


@pytest.mark.parametrize('case', SS.cases(), ids=SS.case_id)
def test_scene_has_on_the_oracle_what_it_is_there_for(lib, case):
    s, allow_sleep = case
    nw, capL, cap = SR.bands(lib, nat, s.N, 0, allow_sleep)
    assert nw >= 2
    E = len(s.envs)
    xy, th, st, ids = SS.plant(s)
    osim = O.OracleSim(O.default_config(E, s.N, allow_sleep=allow_sleep))
    osim.set_poses_m(xy, th)
    if allow_sleep:
        osim.sleep_time[...] = st
    else:
        st = np.zeros_like(st)
    x0, y0 = osim.x.copy(), osim.y.copy()
    rows = []
    for k in range(SS.SINGLE_LAUNCHES):
        before = osim.poses_m()[..., :2].copy()
        osim.set_actions(SS.actions(s, k, st))
        osim.step(1)
        assert int(osim.status.max()) == 0, (s.name, k, osim.status)
        if k == 0:
            after_first = osim.sleep_time.copy() if allow_sleep else None
        row = []
        for e in range(E):
            key, cnt = osim.ws_key[e], osim.ws_cnt[e]
            sizes = SS.islands(key, cnt)
            row.append(dict(contacts=sum(sizes), sizes=sizes, loads=SS.wave_loads(sizes, nw), group=SS.largest_rank_group(key, cnt, before[e]),
                            busiest=SS.busiest_body(key, cnt), pairs=LS.pairs(key, cnt), walls=SS.wall_contacts_of(key, cnt),
                            owner_cnt=cnt.astype(np.int64).copy()))
        rows.append(row)
        print('%s sleep %d launch %d: ' % (s.name, allow_sleep, k) + ' | '.join(
            'contacts %d, largest island %d, waves %s, largest rank group %d, busiest body %d, wall kilobots %d'
            % (f['contacts'], f['sizes'][0], f['loads'], f['group'], f['busiest'], len(f['walls'])) for f in row))
    osim.set_actions(SS.actions(s, SS.SINGLE_LAUNCHES, st))
    osim.step(SS.FUSED_SUBSTEPS)
    assert int(osim.status.max()) == 0, (s.name, 'fused', osim.status)
    for e in range(E):
        col = [r[e] for r in rows]
        for k, f in enumerate(col):
            what = '%s env %d launch %d' % (s.name, e, k)
            assert s.band[0] <= f['contacts'] <= min(s.band[1], capL), (what, f['contacts'])
            assert sum(1 for n in f['sizes'] if n >= 32) <= 1, (what, f['sizes'][:4])        # (wave_loads is exact)
            assert SS.on_register_path(f['sizes'], nw), (what, f['sizes'][:4], f['loads'])
            if 'dealt' in s.has:
                assert max(f['loads']) > SS.LANES, (what, f['loads'])
            if 'single slot' in s.has:
                assert sum(1 for n in f['loads'] if n <= SS.LANES) >= nw - 1, (what, f['loads'])
        first = col[0]
        if 'wave counts' in s.has:
            assert first['loads'] == SS.WAVE_COUNTS_FIRST[e], (e, first['loads'])
            if 'block' in s.envs[e].structs:
                assert all(f['group'] >= SS.RK for f in col), [f['group'] for f in col]
        if 'deep' in s.has:
            assert first['busiest'] >= SS.DEEP, first['busiest']
        if 'rank bucket' in s.has:
            assert first['group'] > SS.RK, first['group']        # ranks RK - 1 and RK: the open-ended bucket runs two rounds
        if 'walls' in s.has:
            w = ids[e]['walls']
            assert all(len(first['walls'].get(int(a), ())) == 1 for a in w[:-1]), first['walls']
            assert len(first['walls'].get(int(w[-1]), ())) == 2, first['walls']
            assert sum(all(int(a) in f['walls'] for a in w) for f in col) >= 3
        if 'normals' in s.has:
            n = ids[e]['normals']
            for a, b in ((n[0], n[1]), (n[2], n[3])):
                assert (int(a), int(b)) in first['pairs'] or (int(b), int(a)) in first['pairs'], (a, b)
            assert x0[e, n[0]] == x0[e, n[1]] and y0[e, n[0]] == y0[e, n[1]]
            dd = float(np.float32(x0[e, n[3]] - x0[e, n[2]]) ** 2 + np.float32(y0[e, n[3]] - y0[e, n[2]]) ** 2)
            assert 1.19209290e-07 ** 2 < dd < 2.0 ** -40, dd
        if 'sleepers' in s.has and allow_sleep:
            z = ids[e]['sleepers']
            assert (osim.sleep_time[e, z] < 0).all()
            inside = set(int(a) for a in z)
            for f in col:
                assert sum(1 for a, b in f['pairs'] if a in inside and b in inside) == 24
    if 'sleepers' in s.has and allow_sleep:
        awake = np.ones((E, s.N), bool)
        for e in range(E):
            awake[e, ids[e]['sleepers']] = False
        assert (after_first[awake] >= 0).all()      # awake ones beside them


def test_the_scenes_select_the_kernels_they_are_there_for(tmp_path):
    from tests import variant_census as VC
    cases = SS.cases()
    listed, selected = VC.host_census(tmp_path, [SR.plan_inputs(s.N, 0, sl) for s, sl in cases])
    for (s, sl), (status, index) in zip(cases, selected):
        drive, light, obj, fn, tier, poly, sense, sleep = listed[index]
        assert status == 0 and (obj, sleep) == (0, sl) and fn == (1024 if s.N == 1024 else 0), (s.name, listed[index])
