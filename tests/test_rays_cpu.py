"""kb_sense_rays and kb_ray_directions without a GPU: the symbols are exported and bound, the direction table is what the
header says, the host-side validation answers in the header's order (arguments before the bound check, so none of it needs
a device), the kernel keeps the keys of its rays in registers (no scratch, no spills in the code object's metadata), and
the numpy restatement (tests/rays_ref.py) is the intended quantity: within a rounding bound of the same formulas in
float64, and within a step of a ray marcher that knows nothing of intersections.  The tie and edge rules are shown on
hand-made cases, and the scenes of tests/test_rays_gpu.py are shown not to be vacuous, on the restatement alone."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from tests import objects_ref
from tests import rays_ref as ref
from tests.host_common import Handle, lib  # noqa: F401
from tests.sensing_common import SWEEP, kernel_metadata, sweep_scene, wall_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RB = 0.0165
f32 = np.float32

# The rounding bound of the float32 evaluation of a ray's t against the same formulas in float64, derived, not observed.
# u = 2^-24 is the unit roundoff of one fp32 operation.  Coordinates are at most 32 world units, so |dx|, |dy| <= 64 and every
# vector from a kilobot to a candidate point, in any frame, is shorter than 128 =: L.
#   (a, l): two products and a sum each, 3 u L, and the library's sine and cosine, within 2 ulp = 2^-22 of the exact ones,
#     times two lengths: 3 u L + 2 x 2^-22 L.
#   (b, q): the error of (a, l) times |u.x| + |u.y| <= sqrt(2); again two products and a sum, 3 u L; and the direction table
#     rounded to fp32, u per component, times two lengths, 2 u L.
#   D := sqrt(2) (3 u L + 2 x 2^-22 L) + 5 u L = 1.57e-4 world units bounds the error of every b and q.
#   Disc: sq = sqrt(r2 - q q) moves by cond x D with cond = |q| / sq (the slope of sq in q), plus a few u r; t = b -+ sq then
#     errs by at most (1 + cond) D + 2 u L.
#   Segment: den = qA - qB errs by 2 D, sg = qA / den (in [0, 1]) by 3 D / |den| + 2 u, and t = bA + sg (bB - bA) by
#     D + 2 D + 3 D |bB - bA| / |den| + 4 u L = (3 + 3 cond) D + 4 u L with cond = |bB - bA| / |den|, the cotangent of the angle
#     at which the ray meets the segment.
# Both are within (3 + 3 cond) D + 4 u L.  The amplification cond has no bound: a grazing ray is ill conditioned, and a hit
# may turn into a miss.  The comparison is made where the float64 winner has cond <= COND_MAX = 2 and both evaluations name
# the same winner; how many rays that leaves out is printed and bounded.
U, L_MAX, COND_MAX = 2.0 ** -24, 128.0, 2.0
D_BQ = math.sqrt(2.0) * (3 * U * L_MAX + 2 * 2.0 ** -22 * L_MAX) + 5 * U * L_MAX
BOUND_WU = (3 + 3 * COND_MAX) * D_BQ + 4 * U * L_MAX
BOUND_M = BOUND_WU / 25.0


def tables(lib, **kw):
    with Handle(lib, **kw) as h:
        return objects_ref.tables(nat.outline(h))


def test_symbols_are_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, 'include', 'kilobots_hip.h')).read()
    for name, nargs in (('kb_sense_rays', 7), ('kb_ray_directions', 2)):
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), name
        assert name in nat.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == nargs
    assert set(re.findall(r'\b(kb_[a-z_]+)\s*\(', hdr)) == set(nat.EXPORTS)
    for define, value in (('KB_RAY_BOTS', nat.RAY_BOTS), ('KB_RAY_OBJECTS', nat.RAY_OBJECTS), ('KB_RAY_WALLS', nat.RAY_WALLS),
                          ('KB_MAX_RAYS', nat.MAX_RAYS)):
        m = re.search(r'#define\s+' + define + r'\s+(\d+)', hdr)
        assert m and int(m.group(1)) == value, define
    assert (nat.RAY_BOTS, nat.RAY_OBJECTS, nat.RAY_WALLS, nat.MAX_RAYS) == (1, 2, 4, 32)
    assert (ref.BOTS, ref.OBJECTS, ref.WALLS) == (nat.RAY_BOTS, nat.RAY_OBJECTS, nat.RAY_WALLS)
    assert 'no reference counterpart' in hdr[hdr.index('Range scans on the CURRENT poses'):hdr.index('int kb_sense_rays')].lower()


@pytest.mark.parametrize('n', range(1, 33))
def test_direction_table_is_the_definition(lib, n):
    buf = (C.c_float * (2 * n + 2))(*([7.0] * (2 * n + 2)))
    assert lib.kb_ray_directions(n, buf) == 0
    assert buf[2 * n] == 7.0 and buf[2 * n + 1] == 7.0          # n rows, nothing behind them
    u = np.array(buf[:2 * n], dtype=np.float32).reshape(n, 2)
    assert nat.ray_directions(n) == [(float(a), float(b)) for a, b in u]
    want = np.array([[f32(math.cos(2.0 * math.pi * k / n)), f32(math.sin(2.0 * math.pi * k / n))] for k in range(n)], dtype=np.float32)
    whole = np.array([(4 * k) % n == 0 for k in range(n)])
    assert np.array_equal(u[~whole].view(np.uint32), want[~whole].view(np.uint32))
    quarter = np.array([(1, 0), (0, 1), (-1, 0), (0, -1)], dtype=np.float32)
    for k in np.flatnonzero(whole):
        assert np.array_equal(u[k], quarter[4 * k // n]) and not np.signbit(u[k][u[k] == 0]).any(), k
    assert np.array_equal(u.view(np.uint32), ref.directions(n).view(np.uint32))
    assert tuple(u[0]) == (1.0, 0.0)                            # ray 0 points dead ahead
    if n >= 3:                                                  # ... and the rays run counter-clockwise
        nxt = np.roll(u.astype(np.float64), -1, 0)
        assert (u[:, 0] * nxt[:, 1] - u[:, 1] * nxt[:, 0] > 0).all()


def test_direction_table_limits(lib):
    buf = (C.c_float * 4)(*([7.0] * 4))
    for n in (0, -1, 33, 64):
        lib.kb_ray_directions(4, None)
        assert lib.kb_ray_directions(n, buf) == nat.KB_EINVAL, n
        assert b'kb_ray_directions' in lib.kb_last_error()
        assert list(buf) == [7.0] * 4
    for n in (1, 8, 32):
        assert lib.kb_ray_directions(n, None) == nat.KB_EINVAL and b'kb_ray_directions' in lib.kb_last_error()
    for n in (0, 33):
        with pytest.raises(nat.KilobotsHipError):
            nat.ray_directions(n)
    assert len(nat.ray_directions(32)) == 32


def test_validation_on_an_unbound_handle(lib):
    """Nothing here launches: the pointers are never dereferenced on the host (any non-NULL value will do).  Every bad call
    has exactly one thing wrong behind the things that are checked before it, and names what it is."""
    dist, hit = C.c_void_p(0x1000), C.c_void_p(0x2000)
    with Handle(lib) as plain, Handle(lib, num_objects=2) as two:
        bad = [
            ('NULL sim', (None, 0.1, 8, 5, dist, hit, None), b'NULL'),
            ('NULL d_dist', (two, 0.1, 8, 5, None, hit, None), b'NULL'),
            ('NULL d_dist before the targets', (two, 0.1, 8, 0, None, hit, None), b'NULL'),
            ('targets = 0', (two, 0.1, 8, 0, dist, hit, None), b'targets'),
            ('targets = 8', (two, 0.1, 8, 8, dist, hit, None), b'targets'),
            ('targets = -1', (two, 0.1, 8, -1, dist, hit, None), b'targets'),
            ('targets before n_rays', (two, 0.1, 0, 15, dist, hit, None), b'targets'),
            ('n_rays = 0', (two, 0.1, 0, 7, dist, hit, None), b'n_rays'),
            ('n_rays = 33', (two, 0.1, 33, 7, dist, hit, None), b'n_rays'),
            ('n_rays before the radius', (two, -1.0, 33, 7, dist, hit, None), b'n_rays'),
            ('radius = 0', (two, 0.0, 8, 7, dist, hit, None), b'radius'),
            ('radius = -1', (two, -1.0, 8, 7, dist, hit, None), b'radius'),
            ('radius = NaN', (two, float('nan'), 8, 7, dist, hit, None), b'radius'),
            ('radius before the objects', (plain, 0.0, 8, 7, dist, hit, None), b'radius'),
            ('objects without objects', (plain, 0.1, 8, 7, dist, hit, None), b'no objects'),
            ('objects alone without objects', (plain, 0.1, 8, 2, dist, None, None), b'no objects'),
        ]
        for what, args, word in bad:
            lib.kb_sense_neighbors(None, 0.07, 8, dist, dist, hit, None)     # (leaves a message that the next call must replace)
            assert lib.kb_sense_rays(*args) == nat.KB_EINVAL, what
            msg = lib.kb_last_error()
            assert msg and b'kb_sense_rays' in msg and word in msg, (what, msg)
        # legal arguments reach the bound check: every subset of the targets, d_hit or not, a radius beyond the arena
        for h, targets in [(two, t) for t in range(1, 8)] + [(plain, t) for t in (1, 4, 5)]:
            for n, r, ph in ((1, 0.1, hit), (32, 100.0, None), (7, 1e-3, hit)):
                assert lib.kb_sense_rays(h, r, n, targets, dist, ph, None) == nat.KB_ENOTBOUND, (targets, n)
                assert b'kb_sense_rays' in lib.kb_last_error() and b'kb_bind' in lib.kb_last_error()


def test_check_rays_and_its_limits():
    assert nat.check_rays(0.1, 8, ('bots', 'walls')) == (0.1, 8, 5)
    assert nat.check_rays(1, 32, 7) == (1.0, 32, 7) and nat.check_rays(0.5, 1, 'objects') == (0.5, 1, 2)
    assert nat.check_rays(0.1, 3, ['walls', 'walls']) == (0.1, 3, 4)
    assert isinstance(nat.check_rays(1, 4.0, 1)[1], int)
    for bad in ((0.0, 8, 7), (-0.1, 8, 7), (float('nan'), 8, 7), (0.1, 0, 7), (0.1, 33, 7), (0.1, 8, 0), (0.1, 8, 8), (0.1, 8, -1),
                (0.1, 8, ()), (0.1, 8, ('bots', 'lights')), (0.1, 8, 'robots'), (0.1, 8, True)):
        with pytest.raises(ValueError):
            nat.check_rays(*bad)
    assert nat.RAY_TARGETS == {'bots': 1, 'objects': 2, 'walls': 4}


def test_batched_env_ray_obs_without_a_gpu():
    import torch
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    from tests.oracle_backend import OracleBackend
    env = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3)
    env.reset()
    a = torch.zeros(3, 16, 2)
    a[..., 0] = 0.01
    assert env.step(a)[3] == {}
    assert env.ray_obs is None
    with pytest.raises(ValueError):
        env.rays()
    for bad in (0.1, (0.1,), (0.1, 8, 'bots', 1), (0.0, 8), (0.1, 0), (0.1, 33), (0.1, 8, ()), (0.1, 8, 'robots'), (0.1, 8, 8),
                (0.1, 8, ('objects',)), (0.1, 8, 7)):
        with pytest.raises(ValueError):
            BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, ray_obs=bad)
    same = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3, ray_obs=None)
    assert same.ray_obs is None and torch.equal(same.reset(), BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3).reset())
    assert same.step(a)[3] == {}
    ok = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3, ray_obs=(0.1, 8))
    assert ok.ray_obs == (0.1, 8, nat.RAY_BOTS | nat.RAY_WALLS)
    assert torch.equal(ok.reset(), BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3).reset())
    assert BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, ray_obs=(0.2, 12, ('walls',))).ray_obs == (0.2, 12, nat.RAY_WALLS)


def test_kernel_uses_no_scratch_and_spills_nothing(lib):
    """The keys of the rays and the carried vertex stay in registers, the tables in LDS: every instantiation (4, 8 and 16
    rays at a time; 17 to 32 rays run the last in two passes) has a zero private segment and zero spill counts in the
    metadata of the code object that was linked."""
    found = kernel_metadata('kb_rays_kernel')
    assert len(found) >= 3, 'kb_rays_kernel: %d instantiations in the code object' % len(found)
    assert {re.search(r'ILi(\d+)E', name).group(1) for name, _ in found} >= {'4', '8', '16'}
    for name, fields in found:
        for key in ('.private_segment_fixed_size', '.sgpr_spill_count', '.vgpr_spill_count'):
            assert fields[key] == 0, (name, key, fields[key])


# ---- the restatement is the intended quantity -----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def forms(lib):
    """The LForm / TForm / CForm / disc scene with 60 kilobots among the shapes and the walls: the outline's tables and the
    float32 state.  The objects stand where tests/test_objects_cpu.py puts them; the kilobots are spread over the arena, a
    cluster around each object and eight along the walls, so that the rays meet kilobots, every object and every wall."""
    tab = tables(lib, **objects_ref.forms_kw())
    rng = np.random.RandomState(17)
    oxy = f32([[12.5, 8.75], [-12.5, 8.75], [-12.5, -8.75], [12.5, -8.75]])
    oth = f32([0.4, -2.1, 1.2, 0.8])
    pts = [oxy[m] + rng.normal(scale=3.0, size=(10, 2)) for m in range(4)]
    pts.append(rng.uniform(-1, 1, size=(12, 2)) * [24.0, 18.0])
    pts.append(np.array([[-24.2, 3.0], [24.3, -5.0], [2.0, 18.1], [-7.0, -18.2], [-24.0, -18.0], [24.1, 18.0], [24.2, -18.1], [-24.3, 18.2]]))
    xy = f32(np.concatenate(pts))
    assert len(xy) == 60 and np.abs(xy).max() <= 32.0
    th = f32(rng.uniform(-np.pi, np.pi, size=len(xy)))
    return dict(tab=tab, state=(xy[:, 0].copy(), xy[:, 1].copy(), th, oxy[:, 0].copy(), oxy[:, 1].copy(), oth))


R_FORMS, K_FORMS = 0.3, 16


def test_restatement_is_within_the_rounding_bound_of_float64(forms):
    """The float32 restatement against the same formulas in float64, bound BOUND_M (derived at the top of this file).  The
    distance of a ray is compared where both evaluations name the same winner and the float64 winner is met at
    cond <= COND_MAX; the others -- grazing rays, and rays on which a near tie or a rounding at t = Rw changes the winner
    -- are counted, printed and must be few."""
    tab, state = forms['tab'], forms['state']
    N = len(state[0])
    d32, h32 = ref.restate_env(tab, *state, R_FORMS, RB, K_FORMS, 7)
    d64, h64, cond = ref.restate_env(tab, *state, R_FORMS, RB, K_FORMS, 7, ft=np.float64, with_cond=True)
    assert d32.dtype == np.float32 and d64.dtype == np.float64 and h32.dtype == np.int32
    same = h32 == h64
    none = same & (h64 < 0)
    assert np.array_equal(d32[none], np.full(none.sum(), f32(R_FORMS) * f32(25) / f32(25)))
    use = same & (h64 >= 0) & (cond <= COND_MAX)
    err = np.abs(d32.astype(np.float64) - d64)
    kinds = [int(((h64 >= 0) & (h64 < N)).sum()), int(((h64 >= N) & (h64 < N + 4)).sum()), int((h64 >= N + 4).sum()), int((h64 < 0).sum())]
    print('%d rays: %d kilobots, %d walls, %d objects, %d nothing; %d compared, largest error %.3g m (bound %.3g m); left out: %d other winner, %d cond > %g'
          % (h64.size, *kinds, use.sum(), err[use].max(), BOUND_M, (~same).sum(), (same & (h64 >= 0) & (cond > COND_MAX)).sum(), COND_MAX))
    assert (err[use] <= BOUND_M).all()
    assert err[use].max() > 0                           # (the bound is not met trivially)
    assert (~same).sum() <= 0.01 * same.size and use.sum() >= 0.5 * (h64 >= 0).sum()
    assert min(kinds) >= 20 and set(range(N + 4, N + 8)) <= set(h64.ravel().tolist()) and set(range(N, N + 4)) <= set(h64.ravel().tolist())


def inside_fixture(fx, oxm, oym, othm, px, py):
    """The points (px, py) (float64 arrays) against one fixture of kb_get_outline standing at (oxm, oym, othm): inside?"""
    c, s = math.cos(float(othm)), math.sin(float(othm))
    dx, dy = px - float(oxm), py - float(oym)
    lx, ly = c * dx + s * dy, c * dy - s * dx
    if fx['n'] == 0:
        return lx * lx + ly * ly <= float(fx['radius']) ** 2
    v = fx['verts'].astype(np.float64)
    ins = np.ones(px.shape, dtype=bool)
    for k in range(fx['n']):
        a, b = v[k], v[(k + 1) % fx['n']]
        ins &= (b[0] - a[0]) * (ly - a[1]) - (b[1] - a[1]) * (lx - a[0]) >= 0
    return ins


def test_restatement_equals_an_independent_ray_marcher(forms):
    """Every ray is marched in 4096 steps of Rw / 4096 against three predicates that know nothing of intersections: inside
    the disc of a kilobot, inside a fixture (cross products with its edges), outside the arena.  A body is crossed at the
    first sample whose answer differs from the answer at the kilobot's own centre -- from inside, that is the way out --
    and the ray's hit is the earliest crossing over all bodies.  The crossing itself then lies in the step before that
    sample: sample - step <= t <= sample for the restatement evaluated in float64 (its float32 evaluation is tied to that
    one by the test above; a step, 1.8e-3 world units, is of the size of that test's bound).  Left out are the rays that
    graze: a disc with ||q| - r| < step, a vertex of a fixture or a corner of the arena within a step of the ray.  There
    the marcher can step over a chord shorter than its step.  Their number is printed."""
    tab, (x, y, th, ox, oy, oth) = forms['tab'], forms['state']
    N, K, S = len(x), K_FORMS, 4096
    Rw = float(f32(R_FORMS) * f32(25))
    rb = float(f32(RB) * f32(25))
    step = Rw / S
    d64, h64 = ref.restate_env(tab, x, y, th, ox, oy, oth, R_FORMS, RB, K, 7, ft=np.float64)
    t_ref = d64 * 25.0
    u = ref.directions(K, np.float64)
    X, Y, TH = x.astype(np.float64), y.astype(np.float64), th.astype(np.float64)
    wdx = np.cos(TH)[:, None] * u[None, :, 0] - np.sin(TH)[:, None] * u[None, :, 1]         # the rays' world directions [N, K]
    wdy = np.sin(TH)[:, None] * u[None, :, 0] + np.cos(TH)[:, None] * u[None, :, 1]
    ts = np.arange(S + 1) * step
    px = X[:, None, None] + wdx[..., None] * ts
    py = Y[:, None, None] + wdy[..., None] * ts
    first = np.full((N, K), S + 1)
    graze = np.zeros((N, K), dtype=bool)

    def cross(ins, skip=None):
        nonlocal first
        change = ins != ins[..., :1]
        n = np.where(change.any(-1), change.argmax(-1), S + 1)
        if skip is not None:
            n[skip] = S + 1
        first = np.minimum(first, n)

    def near(qx, qy, reach):
        """the rays that pass the point within `reach` across and within the range along"""
        dx, dy = qx - X[:, None], qy - Y[:, None]
        b, q = dx * wdx + dy * wdy, dx * wdy - dy * wdx
        return (np.abs(q) < reach) & (b > -reach) & (b < Rw + reach)

    for j in range(N):
        own = np.arange(N) == j
        cross((px - X[j]) ** 2 + (py - Y[j]) ** 2 <= rb * rb, skip=own)
        dx, dy = X[j] - X[:, None], Y[j] - Y[:, None]
        b, q = dx * wdx + dy * wdy, dx * wdy - dy * wdx
        graze |= (np.abs(np.abs(q) - rb) < step) & (b > -rb - step) & (b < Rw + rb + step) & ~own[:, None]
    for fx in tab['fixtures']:
        m = fx['body']
        cross(inside_fixture(fx, ox[m], oy[m], oth[m], px, py))
        c, s = math.cos(float(oth[m])), math.sin(float(oth[m]))
        if fx['n'] == 0:
            dx, dy = float(ox[m]) - X[:, None], float(oy[m]) - Y[:, None]
            b, q = dx * wdx + dy * wdy, dx * wdy - dy * wdx
            r = float(fx['radius'])
            graze |= (np.abs(np.abs(q) - r) < step) & (b > -r - step) & (b < Rw + r + step)
        for vx, vy in fx['verts'].astype(np.float64):
            graze |= near(float(ox[m]) + c * vx - s * vy, float(oy[m]) + s * vx + c * vy, step)
    x0, x1, y0, y1 = (float(v) for v in tab['arena'])
    cross((px < x0) | (px > x1) | (py < y0) | (py > y1))
    for cx in (x0, x1):
        for cy in (y0, y1):
            graze |= near(cx, cy, step)
    hit_m = first <= S
    t_m = first * step
    use = ~graze
    print('%d rays, %d graze a body and are left out; of the others %d hit something, largest sample - t = %.3g steps, smallest %.3g'
          % (graze.size, graze.sum(), (hit_m & use).sum(), ((t_m - t_ref)[hit_m & use] / step).max(), ((t_m - t_ref)[hit_m & use] / step).min()))
    eps = 1e-9
    # a crossing in the very last step may lie beyond Rw: the marcher then sees a hit at its last sample where there is none
    edge = use & hit_m & (h64 < 0) & (first == S)
    agree = use & ~edge
    assert np.array_equal(hit_m[agree], (h64 >= 0)[agree])
    both = agree & hit_m
    assert (t_ref[both] <= t_m[both] + eps).all() and (t_ref[both] >= t_m[both] - step - eps).all()
    assert use.sum() >= 0.9 * use.size and both.sum() >= 0.5 * use.size and edge.sum() <= 2


# ---- ties and edges, on the restatement -------------------------------------------------------------------------------------
ARENA = f32([-25, 25, -18.75, 18.75])
Z = np.zeros(0, dtype=np.float32)


def scan(xy, th, n_rays, targets, R=0.2, tab=None, objects=(Z, Z, Z)):
    tab = tab or dict(M=0, arena=ARENA, fixtures=[])
    xy = f32(xy)
    return ref.restate_env(tab, xy[:, 0].copy(), xy[:, 1].copy(), f32(th), *objects, R, RB, n_rays, targets)


def test_a_ray_through_a_vertex_meets_both_edges():
    """An axis-aligned box of half extents (2, 1) at the origin and a kilobot at (-4, -3) heading along x: ray 1 of 8 is the
    exact diagonal and runs through the vertex (-2, -1), q = 0 for both edges that meet there.  Both straddle; the edge
    that starts at the vertex gives t = b exactly (sg = 0), and that is what the ray reports."""
    tab = dict(M=1, arena=ARENA, fixtures=[dict(body=0, kind=1, n=4, radius=f32(0), verts=f32([[-2, -1], [2, -1], [2, 1], [-2, 1]]))])
    u = ref.directions(8)
    assert u[1, 0] == u[1, 1]
    d, h = scan([[-4.0, -3.0]], [0.0], 8, ref.OBJECTS, tab=tab, objects=(f32([0]), f32([0]), f32([0])))
    b = f32(2) * u[1, 0] + f32(2) * u[1, 1]
    assert h[0, 1] == 1 + 4 + 0 and d[0, 1] == b / f32(25)
    tA, okA, _ = ref.segment(b, f32(0), f32(6) * u[1, 0] + f32(2) * u[1, 1], f32(6) * u[1, 1] - f32(2) * u[1, 0])       # (-2, -1) -> (2, -1)
    tB, okB, _ = ref.segment(f32(2) * u[1, 0] + f32(4) * u[1, 1], f32(2) * u[1, 1] - f32(4) * u[1, 0], b, f32(0))       # (-2, 1) -> (-2, -1)
    assert okA and okB and tA == b and abs(float(tB) - float(b)) <= 4 * 2.0 ** -24 * float(b)
    assert h[0, 0] == -1 and d[0, 0] == f32(0.2) * f32(25) / f32(25)       # ray 0 passes below the box


def test_a_ray_through_an_arena_corner_goes_to_the_lower_wall():
    """From (xmin + 3, ymin + 3), heading along x, ray 5 of 8 is the exact diagonal into the corner (xmin, ymin), where W0 and
    W2 both start: q = 0, sg = 0, t = b for both.  Equal t: the lower code wins.  Each alone reports the same distance."""
    xy = [[-22.0, -15.75]]
    u = ref.directions(8)
    assert u[5, 0] == u[5, 1] < 0
    d, h = scan(xy, [0.0], 8, ref.WALLS)
    b = f32(-3) * u[5, 0] + f32(-3) * u[5, 1]
    assert h[0, 5] == 1 + 0 and d[0, 5] == b / f32(25)
    t0, ok0, _ = ref.segment(b, f32(0), f32(-3) * u[5, 0] + f32(34.5) * u[5, 1], f32(-3) * u[5, 1] - f32(34.5) * u[5, 0])      # W0
    t2, ok2, _ = ref.segment(b, f32(0), f32(47) * u[5, 0] + f32(-3) * u[5, 1], f32(47) * u[5, 1] - f32(-3) * u[5, 0])          # W2
    assert ok0 and ok2 and t0 == t2 == b
    assert h[0, 4] == 1 + 0 and d[0, 4] == f32(3) / f32(25) and h[0, 6] == 1 + 2 and d[0, 6] == f32(3) / f32(25)
    assert h[0, 0] == -1


def test_equal_t_goes_to_the_lower_kilobot():
    """Kilobots 1 and 2 mirrored about ray 0 of kilobot 0: the same q^2, the same t; then the same with the indices swapped."""
    for first, second in ((0.2, -0.2), (-0.2, 0.2)):
        d, h = scan([[0.0, 0.0], [3.0, first], [3.0, second]], [0.0, 1.0, 2.0], 4, ref.BOTS)
        q2 = f32(0.2) * f32(0.2)
        rb = f32(RB) * f32(25)
        t = f32(3) - np.sqrt(rb * rb - q2)
        assert h[0, 0] == 1 and d[0, 0] == t / f32(25)
        assert list(h[0, 1:]) == [-1, -1, -1]


def test_coincident_and_touching_kilobots_and_one_outside_the_arena():
    rb = f32(RB) * f32(25)
    # 0 and 1 on one point: dd = 0, the origin is inside the other's disc, t1 = -rb < 0, t = t2 = rb on every ray
    # 2 and 3: 3 touches 2 dead ahead of it, at 2 rb: t1 = 2 rb - rb = rb
    # 4: a step outside the xmax wall, heading along x: the ray astern meets W1 from behind, the others nothing
    xy = [[-10.0, 5.0], [-10.0, 5.0], [0.0, -6.0], [float(rb + rb), -6.0], [26.0, 0.5]]
    d, h = scan(xy, [0.7, -2.0, 0.0, 0.0, 0.0], 4, ref.BOTS | ref.WALLS)
    assert list(h[0]) == [1, 1, 1, 1] and list(h[1]) == [0, 0, 0, 0]
    assert (d[:2] == rb / f32(25)).all()
    assert f32(xy[3][0]) - f32(0.0) == rb + rb and np.sqrt(rb * rb) == rb
    assert h[2, 0] == 3 and d[2, 0] == rb / f32(25) and h[3, 2] == 2 and d[3, 2] == rb / f32(25)
    assert h[4, 2] == 5 + 1 and d[4, 2] == f32(1) / f32(25)
    assert list(h[4, [0, 1, 3]]) == [-1, -1, -1] and (d[4, [0, 1, 3]] == f32(0.2) * f32(25) / f32(25)).all()
    # kilobots only: the one outside sees nothing at all
    d, h = scan(xy, [0.7, -2.0, 0.0, 0.0, 0.0], 4, ref.BOTS)
    assert (h[4] == -1).all()


# ---- the scenes of tests/test_rays_gpu.py are not vacuous --------------------------------------------------------------------
def plain_tab(lib):
    tab = tables(lib)
    assert tab['M'] == 0 and list(tab['arena']) == [-25.0, 25.0, -18.75, 18.75]
    return tab


@pytest.mark.parametrize('E,N,R', SWEEP)
def test_sweep_scenes_are_not_vacuous(lib, E, N, R):
    """With the kilobots as the only targets at least one ray hits a kilobot and at least one hits nothing, in every scene of
    more than one kilobot (1024 kilobots: the first env alone shows it); a lone kilobot hits nothing.  With the walls, the
    scene whose radius spans the arena hits something on every ray; with the walls alone, a wall on every ray, and all four."""
    tab = plain_tab(lib)
    x, y, th = ref.world(*sweep_scene(E, N))
    envs = range(1 if N == 1024 else E)
    hits = np.stack([ref.restate_env(tab, x[e], y[e], th[e], Z, Z, Z, R, RB, 8, ref.BOTS)[1] for e in envs])
    share = (hits >= 0).mean()
    print('(%d, %d, %g): %.0f %% of the rays hit a kilobot' % (E, N, R, 100 * share))
    if N == 1:
        assert share == 0
    else:
        assert 0 < share < 1 and hits.max() < N
    if R == 4.0:
        both = np.stack([ref.restate_env(tab, x[e], y[e], th[e], Z, Z, Z, R, RB, 8, ref.BOTS | ref.WALLS)[1] for e in envs])
        walls = np.stack([ref.restate_env(tab, x[e], y[e], th[e], Z, Z, Z, R, RB, 8, ref.WALLS)[1] for e in envs])
        assert (both >= 0).all() and (both >= N).any() and (both < N).any()
        assert (walls >= N).all() and set(walls.ravel().tolist()) == {N, N + 1, N + 2, N + 3}


@pytest.mark.parametrize('R', [0.04, 0.15])
def test_the_wall_scene_reports_all_four_walls(lib, R):
    tab = plain_tab(lib)
    x, y, th = ref.world(*wall_scene(random_headings=True))
    N = x.shape[1]
    hits = np.stack([ref.restate_env(tab, x[e], y[e], th[e], Z, Z, Z, R, RB, 8, ref.BOTS | ref.WALLS)[1] for e in range(4)])
    seen = set(hits.ravel().tolist())
    print('R = %g: %d rays on a wall, %d on a kilobot, %d on nothing' % (R, (hits >= N).sum(), ((hits >= 0) & (hits < N)).sum(), (hits < 0).sum()))
    assert {N, N + 1, N + 2, N + 3} <= seen and -1 in seen and min(seen - {-1}) < N


@pytest.mark.parametrize('name', sorted(ref.OBJECT_SEEDS))
def test_object_scenes_hit_every_object(lib, name):
    kw, xy, th, objs, oth = ref.object_scene(name)
    S = ref.OBJECT_SCENE
    tab = tables(lib, E=S['E'], N=S['N'], **kw)
    x, y, t = ref.world(xy, th)
    ox, oy, ot = ref.world(objs, oth)
    N, M = S['N'], tab['M']
    for targets in (7, ref.OBJECTS):
        hits = np.stack([ref.restate_env(tab, x[e], y[e], t[e], ox[e], oy[e], ot[e], S['R'], RB, S['K'], targets)[1] for e in range(S['E'])])
        seen = set(hits.ravel().tolist())
        print('%s, targets %d: %d rays on an object, %d on nothing' % (name, targets, (hits >= N + 4).sum(), (hits < 0).sum()))
        assert set(range(N + 4, N + 4 + M)) <= seen, (name, targets)
    assert -1 in seen
