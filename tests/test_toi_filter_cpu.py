"""The rule by which the step kernels decide who enters the continuous step against the walls (tests/toi_scenes.py: no_event),
proved on the oracle: for every kilobot and substep in which the rule says "no wall can have an event", the oracle's state
with and without the continuous step (its toi_walls switch) is the same bit pattern.

Two oracles run in lockstep.  Before each substep the one without the continuous step takes over the whole state of the one
with it, so that its result is the pose behind the position sweeps -- the end of the sweep that kb_toi_wall looks at -- and the
state before the substep is its start.  The scenes must not be vacuous: events on every wall and in a corner, kilobots that
rest inside `total` (which the quick reject that was there before let through) and are rejected now, every branch of the rule
deciding, start and end distances on both sides of tt and of `total`, on tt itself where tt is an fp32 wall distance, and
env-substeps with and without a candidate (counted as the kernel counts them: awake behind the substep's sleep bookkeeping, not
rejected) among the single launches of tests/test_toi_filter_gpu.py and inside its fused launch, both for one env inside it --
without a candidate the kernels go round the processing loop and its barriers."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import toi_scenes as TS
from tests.host_common import word_bits

f32 = TS.f32
FIELDS = ('x', 'y', 'theta', 'v', 'w', 'sleep_time')


def lockstep(s, allow_sleep):
    """per substep: (awake [E, N], d0, d1 [4, E, N], differs [E, N], with, without) -- `differs`: the continuous step changed
    some field of the kilobot"""
    xy, th, acts, st, ids = TS.plant(s)
    E = xy.shape[0]
    sims = []
    for toi in (1, 0):
        o = O.OracleSim(O.default_config(E, s.N, O.DRIVE_VELOCITY, O.LIGHT_NONE, bot_radius=s.radius, toi_walls=toi, allow_sleep=allow_sleep))
        o.set_poses_m(xy, th)
        if allow_sleep:
            o.sleep_time[...] = st
        sims.append(o)
    a, b = sims
    for k in range(TS.SUBSTEPS):
        for name, _t in O.State._fields_:
            if getattr(a, name, None) is not None:
                getattr(b, name)[...] = getattr(a, name)
        x0, y0 = a.x.copy(), a.y.copy()
        awake = ~(a.sleep_time < 0) if allow_sleep else np.ones(x0.shape, bool)
        for o in sims:
            o.set_actions(acts)                 # (the sleepers are never commanded)
            o.step(1)
        d0, d1 = TS.sweep_dists(x0, y0, b.x, b.y)
        differs = np.zeros(x0.shape, bool)
        for f in FIELDS:
            differs |= word_bits(getattr(a, f)) != word_bits(getattr(b, f))
        assert np.array_equal(a.ws_cnt, b.ws_cnt) and np.array_equal(a.ws_key, b.ws_key) and np.array_equal(word_bits(a.ws_acc), word_bits(b.ws_acc))
        collected = ~(a.sleep_time < 0) if allow_sleep else awake       # the collection looks behind the substep's sleep bookkeeping
        yield k, awake, d0, d1, differs, x0, y0, b, collected
    assert int(a.status.max()) == 0 and int(b.status.max()) == 0


@pytest.mark.parametrize('case', TS.cases(), ids=TS.case_id)
def test_rejected_kilobots_leave_the_continuous_step_as_they_came(case):
    s, allow_sleep = case
    total, tt = TS.thresholds(s.radius)
    on_grid = float(tt) / TS.GRID == round(float(tt) / TS.GRID)
    assert on_grid == (s.N != 1024)
    events, corner_events, saved, branch = np.zeros(4, int), 0, np.zeros(4, int), np.zeros(4, int)
    unrest = 0
    seen = {k: set() for k in ('d0-tt', 'd1-tt', 'd0-total', 'd1-total')}
    ids = TS.plant(s)[4]
    ncand = []
    for k, awake, d0, d1, differs, x0, y0, b, collected in lockstep(s, allow_sleep):
        ne = TS.no_event(d0, d1, tt)
        rejected = ne.all(0)
        ncand.append((~rejected & collected).sum(1))        # candidates per env, as the kernel counts them
        bad = rejected & differs
        assert not bad.any(), '%s, substep %d: the rule rejects kilobot %s, and the continuous step changes it (d0 %s, d1 %s)' % (
            s.name, k, np.argwhere(bad)[0], d0[(slice(None),) + tuple(np.argwhere(bad)[0])], d1[(slice(None),) + tuple(np.argwhere(bad)[0])])
        # ---- what the scene has ----
        ev = differs
        open_ = ~ne
        for wl in range(4):
            events[wl] += int((ev & open_[wl] & (open_.sum(0) == 1)).sum())
            saved[wl] += int((rejected & awake & (d0[wl] <= total) & TS.old_reject_passes(x0, y0, b.x, b.y, total)).sum())
        corner_events += int((ev & (open_.sum(0) >= 2)).sum())
        with np.errstate(invalid='ignore'):
            touching = np.abs(d0) < tt
            branch += [int((np.abs(d0) <= 0).sum()), int((touching & ~(np.abs(d0) <= 0)).sum()),
                       int((~touching & (d1 > tt)).sum()), int((~touching & ~(d1 > tt)).sum())]
        step = lambda d, ref: set(np.unique((d[np.abs(d - ref) < 3 * TS.GRID].astype(np.float64) - float(ref)) / TS.GRID))      # noqa: E731
        seen['d0-tt'] |= step(d0, tt)
        seen['d1-tt'] |= step(d1[~touching], tt)            # (the end distance decides where the start does not touch)
        seen['d0-total'] |= step(d0, total)
        seen['d1-total'] |= step(d1, total)
        # the pressed kilobots rest: inside `total`, outside tt, for every substep
        for e, where in enumerate(ids):
            p = np.concatenate([where.get('pressed', np.zeros(0, int)), where.get('pressed corner', np.zeros(0, int))])
            unrest += int((~((d0[:, e, p].min(0) <= total) & rejected[e, p])).sum())
    print('%s: events per wall %s, in a corner %d; rejected inside `total` per wall %s; branches %s; seen %s' % (
        s.name, events, corner_events, saved, branch, {k: sorted(v) for k, v in seen.items()}))
    assert (saved > 0).all(), saved
    # the kernels go round the processing loop and its barriers where an env-substep has no candidate: both ways among the
    # single launches, both inside the fused launch, and both for ONE env inside the fused launch
    ncand = np.array(ncand)                                  # [substep, env]
    single, fused = ncand[:TS.SINGLE_LAUNCHES], ncand[TS.SINGLE_LAUNCHES:]
    print('%s: candidates per env-substep\n%s' % (s.name, ncand.T))
    for name, part in (('single launches', single), ('fused launch', fused)):
        assert (part == 0).any() and (part > 0).any(), '%s: %s' % (name, part.T)
    assert any((fused[:, e] == 0).any() and (fused[:, e] > 0).any() for e in range(ncand.shape[1])), fused.T
    assert (branch > 0).all(), 'a branch of the rule never decided: %s' % branch
    assert unrest == 0, 'a pressed kilobot left the skin of its wall or became a candidate in %d kilobot-substeps' % unrest
    if s.N == 16:
        assert events.sum() > 0 and corner_events > 0, (events, corner_events)      # (one wall per env carries the thresholds)
    else:
        assert (events > 0).all() and corner_events > 0, (events, corner_events)
    # both sides of each threshold, in fp32 steps of the wall distance (tt on the grid: the threshold itself as well)
    for key in ('d0-tt', 'd1-tt'):
        assert min(seen[key]) < 0 < max(seen[key]), (key, seen[key])
        assert (0.0 in seen[key]) == on_grid, (key, seen[key])
    for key in ('d0-total', 'd1-total'):
        assert min(seen[key]) <= 0 < max(seen[key]), (key, seen[key])


def test_threshold_is_the_sum_kb_toi_wall_compares_with():
    """tt, as the scenes evaluate it, against fmaxf(slop, total - 3 slop) + 0.25 slop evaluated a
    second way: every operation in float64 on float32 operands, rounded to float32 (53 >= 2 * 24 + 2 digits: rounding twice
    is rounding once).  total - 2.75 slop, the closed form, is a different float for some radii -- the sum is the rule.
    This holds the SCENES' threshold.  The value the host computes for the kernels (Params::toi_tt in kb_create) is not
    exposed by the handle: what holds it are the kilobots of tests/test_toi_filter_gpu.py one fp32 step either side of tt and
    on it, at two radii -- a host value off by one unit in the last place collects or drops one of them against the oracle."""
    closed_form_differs = 0
    for radius in (TS.DEFAULT_RADIUS, TS.grid_radius(), 0.03, 0.01, 0.0001, 0.05):
        total, tt = TS.thresholds(radius)
        r = f32(float(f32(radius)) * 25.0)
        tot = f32(float(r) + float(f32(2.0 * float(f32(0.005)))))
        target = max(f32(0.005), f32(float(tot) - float(f32(3.0 * float(f32(0.005))))))
        want = f32(float(target) + float(f32(0.25 * float(f32(0.005)))))
        assert word_bits(tot) == word_bits(total) and word_bits(want) == word_bits(tt), (radius, total, tt, tot, want)
        closed_form_differs += int(f32(total - f32(2.75) * f32(0.005)).tobytes() != tt.tobytes())
    assert float(TS.thresholds(0.0001)[1]) == float(f32(0.005) + f32(0.25) * f32(0.005))      # the fmaxf decides for a tiny body
    print('total - 2.75 slop differs from the sum for %d of 6 radii' % closed_form_differs)
