"""The scenes of tests/packed_round_scenes.py without a GPU: on the oracle every case has, in the launches that
tests/test_packed_rounds_gpu.py runs, what it is there for -- a wave of more than 64 contacts beside one of at most 64, a
contact on each of the four walls, a corner, a flipped wall normal, contacts four levels deep --, stays on the register path
and ends every launch with status 0.  These are conditions on the scenes, not measurements."""
import numpy as np
import pytest

from tests import packed_round_scenes as PR
from tests import setup_scenes as SS
from tests import solver_regimes as SR
from tests import variant_census as VC

PM = PR.PM


def test_the_cases_cover_both_sleep_settings_and_both_continuous_settings():
    assert len(PR.CASES) == 16 and PR.launches() == [1] * 6 + [10]
    for name in ('slots-1024', 'walls-1024', 'deep-1024', 'rich-200'):
        assert {(sl, toi) for n, sl, toi in PR.CASES if n == name} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        N, xy, th, actions, driven = PR.start(name)
        assert xy.shape[0] == 2 and N == (200 if name == 'rich-200' else 1024)
    # the wall kilobots in the numbers the kernel sees: inside the skin of their walls, the last one beyond the left wall
    N, xy, th, actions, driven = PR.start('walls-1024')
    for e in range(2):
        p = xy[e, driven[e]]
        assert (np.abs(p[:6]) <= [1.0, 0.75]).all() and p[PR.OUTSIDE, 0] < -1.0
        assert len(set(map(int, driven[e]))) == len(PR.WALL_PLACES)
        a = actions(0)
        assert (a[e, driven[e], 0] > 0).all() and (a[e, driven[e], 1] == 0).all()


@pytest.mark.parametrize('case', PR.CASES, ids=PR.case_id)
def test_case_has_on_the_oracle_what_it_is_there_for(case):
    name, sleep, toi = case
    s = PR.scene_of(name)
    N, xy, th, actions, driven = PR.start(name)
    nw = 8 if N == 1024 else 2
    ref = PR.reference(case)
    assert len(ref) == PR.SINGLE_LAUNCHES + 1
    for k, (snap, facts, x0, y0) in enumerate(ref):
        what = '%s launch %d' % (PR.case_id(case), k)
        assert int(snap.status.max()) == 0, (what, snap.status)
        assert int(snap.ws_cnt.astype(np.int64).sum(1).min()) > 0, what
        if facts is None:
            continue
        print(what, [(f.ncon, f.largest, f.rule, f.loads, f.depth, sorted((a, sorted(w)) for a, w in f.walls.items() if len(w) > 1 or 'walls' in s.has))
                     for f in facts])
        for e, f in enumerate(facts):
            # the register path: no island for the cooperative sweep, no wave above its two slots
            assert 0 < f.largest <= SS.GIANT_ISLAND and max(f.loads) <= PM.WAVE, (what, e, f.largest, f.loads)
            if 'slots' in s.has:
                assert f.rule == 'packed' and max(f.loads) > PM.SLOT and any(0 < c <= PM.SLOT for c in f.loads), (what, e, f.loads)
            if 'walls' in s.has:
                touched = set().union(*f.walls.values())
                assert touched == {0, 1, 2, 3}, (what, e, touched)
                assert all(int(a) in f.walls for a in driven[e]), (what, e, f.walls)
                assert all(len(f.walls[int(a)]) == 2 for a in driven[e][4:6]), (what, e, f.walls)         # the corners
                # the kilobot beyond the left wall: its centre is outside at the start of the substep, so the normal is flipped
                out = int(driven[e][PR.OUTSIDE])
                assert x0[e, out] < np.float32(-1.0 * SS.WORLD) and 0 in f.walls[out], (what, e, x0[e, out])
            if 'deep' in s.has:
                assert f.depth >= PR.MIN_DEPTH, (what, e, f.depth)
            if 'rich' in s.has:
                assert f.ncon > PM.SLOT and f.depth >= PR.MIN_DEPTH and f.walls, (what, e, f.ncon, f.depth)


def test_the_scenes_select_the_kernels_they_are_there_for(tmp_path):
    listed, selected = VC.host_census(tmp_path, [SR.plan_inputs(PR.start(name)[0], 0, sl) for name, sl, toi in PR.CASES])
    for (name, sl, toi), (status, index) in zip(PR.CASES, selected):
        drive, light, obj, fn, tier, poly, sense, sleep = listed[index]
        assert status == 0 and (obj, sleep) == (0, sl) and fn == (1024 if PR.start(name)[0] == 1024 else 0), (name, listed[index])
        assert sense == 0 or fn == 0, (name, listed[index])      # (the generic kernels carry the sensing pass as a run-time branch)
