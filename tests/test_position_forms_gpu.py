"""The position sweep of the register solver with the short forms of kb_exact.h, bit for bit against the oracle: 10
single-substep launches per scene, with and without the sleep state.  x, y and theta are compared as bit patterns as well:
the sign of a zero is part of the result.

  (a) 8 kilobots x 64 envs around every branch of the round: two coincident kilobots (len == 0: outside the guard, the
      branch for coincident centres), a pair overlapping so deep that C reaches -B2_MAX_LINEAR_CORRECTION, a pair that
      touches inside the slop (C = fminf(positive, 0) = +0: the quotient -C / K is -0) spawned on x = -0.0 (a control run of
      the oracle shows in which envs the contact meets x = -0, and there the bit of x depends on the quotient's sign), a kilobot in a corner
      on two walls (K = im_bot) and one beyond a wall line.  Kilobots of 0.03 m radius: a pair of the default 0.0165 m
      cannot overlap by B2_MAX_LINEAR_CORRECTION / B2_BAUMGARTE = 1 world unit.  kb_create checks the division for this K.
      (sep + B2_LINEAR_SLOP == 0 EXACTLY has no fp32 solution at either radius: sep is the exact difference of numbers with
      ulp >= 2^-25, 0.005f is no multiple of that.  C == 0 needs no such accident: every contact that rests within the slop has it.)
  (b) 1024 kilobots x 4 envs of the 1024-p042 scene of tests/solver_regimes.py: the fixed-size instantiation, every substep
      on the register path, the default configuration's K.
  (c) pairs whose centres are 2^-21 .. 2^-25 world units apart: dd below the guard's 2^-40, the whole wave takes the IEEE
      sequences (a finite configuration outside the guard exists, so the scene stays).  What this scene cannot show is that
      the fall-back WAS taken: just below 2^-40 the short forms most likely give the same bits.  The pair that depends on
      the guard is the coincident one of (a): v_rsq_f32(0) is infinite and the short forms would return NaN."""
import numpy as np
import pytest

from tests import solver_regimes as SR
from tests.gpu_common import make_pair, assert_same, assert_ws_same, cpu, dev

pytestmark = pytest.mark.gpu

LAUNCHES = 10
WS = 25.0
XMAX, YMAX = 25.0, 18.75
SLOP, BAUMGARTE, MAX_CORR = np.float32(0.005), np.float32(0.2), np.float32(0.2)
f32 = np.float32


def assert_same_bits(osim, gsim, what):
    """assert_same compares values, and -0.0 == +0.0: the sign of a zero is only seen in the bit patterns"""
    for f in ('x', 'y', 'theta'):
        a, b = getattr(osim, f), cpu(getattr(gsim, f)).reshape(getattr(osim, f).shape)
        diff = a.view(np.uint32) != b.view(np.uint32)
        assert not diff.any(), '%s: %s differs in its bits at %s: oracle %r, device %r' % (
            what, f, np.argwhere(diff)[0], a[diff][0], b[diff][0])


def run(osim, gsim, E, N, allow_sleep, what, moving=None, after=None):
    fields = ('x', 'y', 'theta') + (('sleep_time',) if allow_sleep else ())
    for k in range(LAUNCHES):
        a = SR.actions(E, N, k)
        if moving is not None:
            a[:, ~moving] = 0.0
        osim.set_actions(a)
        osim.step(1)
        gsim.step(1, actions=dev(a))
        assert_same(osim, gsim, '%s, substep %d' % (what, k), fields)
        assert_same_bits(osim, gsim, '%s, substep %d' % (what, k))
        assert_ws_same(osim, gsim, '%s, substep %d' % (what, k))
        if after is not None:
            after(k)
    assert int(osim.status.max()) == 0 and int(cpu(gsim.status).max()) == 0


def make_oracle(E, N, xy, th, **kw):
    from oracle import oracle as O
    o = O.OracleSim(O.default_config(E, N, O.DRIVE_VELOCITY, O.LIGHT_NONE, **kw))
    o.set_poses_m(xy, th)
    return o


@pytest.mark.parametrize('allow_sleep', [0, 1], ids=['nosleep', 'sleep'])
def test_a_every_branch_of_the_round(allow_sleep):
    E, N, radius = 64, 8, 0.03
    r = f32(radius) * f32(WS)
    rng = np.random.RandomState(11)
    x = np.zeros((E, N)); y = np.zeros((E, N))
    x[:, 0:2], y[:, 0:2] = 7.5, 5.0                                           # coincident
    x[:, 2], y[:, 2], x[:, 3], y[:, 3] = -10.0, 5.0, -10.0 + 0.25, 5.0        # sep = 0.25 - 1.5 < -(1 + slop): C is clamped
    assert BAUMGARTE * (f32(0.25) - r - r + SLOP) < -MAX_CORR
    x[:, 4:6] = -0.0                                                          # touching inside the slop: C = fminf(positive, 0) = +0, -C / K = -0
    y[:, 4], y[:, 5] = -7.5, -7.5 + 1.5 - 0.002
    sep = f32(f32(y[0, 5]) - f32(y[0, 4])) - r - r
    assert sep < 0 and sep + SLOP > 0
    x[:, 6], y[:, 6] = XMAX - 0.74, YMAX - 0.74                               # corner: on two walls
    x[:, 7], y[:, 7] = -XMAX - 0.5, rng.uniform(-10.0, 10.0, E)               # beyond the left wall line
    x[:, 6] -= rng.uniform(0.0, 0.01, E)                                      # the envs differ
    th = rng.uniform(-np.pi, np.pi, (E, N))
    assert np.signbit(f32(x[0, 4])) and f32(x[0, 4]) == 0.0
    osim, gsim = make_pair(E, N, xy=np.stack([x, y], -1) / WS, th=th, allow_sleep=allow_sleep, bot_radius=radius)
    assert gsim._lib.kb_exact_division(gsim._h) == 1
    assert np.signbit(osim.x[0, 4]) and np.signbit(cpu(gsim.x)[0, 4])
    moving = np.ones(N, bool)
    moving[4:6] = False            # the pair at rest stays where its separation is exact
    # The state in which the sign of the zero quotient decides a bit.  A control oracle has kilobot 5 one unit further up,
    # so the pair does not touch and x of kilobot 4 after the first substep is what the integration left: -0 + h * vx, -0
    # wherever the commanded vx is a negative zero.  In those envs the contact turns it into -0 - im * (-0 * nx) = +0; with
    # a quotient of +0 (the plain fma form, or `K > 0 ? form : 0`) it would stay -0 - (+0) = -0, and stays so in later substeps.
    y_apart = y.copy()
    y_apart[:, 5] += 1.0
    control = make_oracle(E, N, np.stack([x, y_apart], -1) / WS, th, allow_sleep=allow_sleep, bot_radius=radius)

    def zero_signs(k):
        if k == 0:
            a = SR.actions(E, N, 0)
            a[:, ~moving] = 0.0
            control.set_actions(a)
            control.step(1)
            sensitive = np.signbit(control.x[:, 4]) & (control.x[:, 4] == 0.0)
            assert sensitive.sum() >= E // 4, 'only %d envs reach the contact with x = -0' % sensitive.sum()
            zero_signs.sensitive = sensitive
        for sim_x in (osim.x[:, 4], cpu(gsim.x).reshape(osim.x.shape)[:, 4]):
            assert (sim_x[zero_signs.sensitive] == 0.0).all() and not np.signbit(sim_x[zero_signs.sensitive]).any()
    run(osim, gsim, E, N, allow_sleep, '(a) sleep %d' % allow_sleep, moving, zero_signs)


@pytest.mark.parametrize('allow_sleep', [0, 1], ids=['nosleep', 'sleep'])
def test_b_fixed_size_kernel_on_the_register_path(allow_sleep):
    s = next(s for s in SR.SCENES if s.name == '1024-p042')
    E = 4
    xy, th = SR.start(s, E)
    osim, gsim = make_pair(E, s.N, xy=xy, th=th, **SR.config_kw(s, allow_sleep))
    assert gsim._lib.kb_exact_division(gsim._h) == 1
    band = (gsim.block_threads // SR.LANES, gsim.lds_staging_entries, gsim.contact_capacity)
    fields = ('x', 'y', 'theta') + (('sleep_time',) if allow_sleep else ())
    # the lattice closes up under the drive and has few contacts before substep 8: the scene's own 12 substeps, not 10
    assert s.substeps >= LAUNCHES
    for k in range(s.substeps):
        a = SR.actions(E, s.N, k)
        osim.set_actions(a)
        osim.step(1)
        gsim.step(1, actions=dev(a))
        what = '(b) sleep %d, substep %d' % (allow_sleep, k)
        assert_same(osim, gsim, what, fields)
        assert_ws_same(osim, gsim, what)
        assert set(SR.classify(cpu(gsim.ws_cnt), band)) == {'R0'}, what
    assert SR.counts(cpu(gsim.ws_cnt)).min() >= SR.R0_MIN_CONTACTS
    assert int(osim.status.max()) == 0 and int(cpu(gsim.status).max()) == 0


@pytest.mark.parametrize('allow_sleep', [0, 1], ids=['nosleep', 'sleep'])
def test_c_lengths_below_the_guard_take_the_ieee_sequences(allow_sleep):
    E, N = 16, 8
    rng = np.random.RandomState(12)
    x = np.zeros((E, N)); y = np.zeros((E, N))
    for pair, gap in enumerate((2.0 ** -21, 2.0 ** -23, 2.0 ** -25, 0.8)):     # the last pair: an ordinary contact in the same wave
        x[:, 2 * pair] = 0.25                  # (fp32 resolves 2^-25 next to 0.25)
        x[:, 2 * pair + 1] = 0.25 + gap
        y[:, 2 * pair] = y[:, 2 * pair + 1] = -9.0 + 6.0 * pair + rng.uniform(-1.0, 1.0, E)
    dx = f32(x[:, 1]) - f32(x[:, 0])
    assert (dx > 0).all() and (dx * dx < 2.0 ** -40).all()                      # nonzero, and below the guard
    th = rng.uniform(-np.pi, np.pi, (E, N))
    osim, gsim = make_pair(E, N, xy=np.stack([x, y], -1) / WS, th=th, allow_sleep=allow_sleep)
    run(osim, gsim, E, N, allow_sleep, '(c) sleep %d' % allow_sleep)
