"""kb_sense_objects and kb_get_outline without a GPU: the symbols are exported and bound, the host-side validation answers
in the header's order (arguments before the bound check, so none of it needs a device), the kernel has no private segment
and no spill (the code object's metadata), kb_get_outline returns the fixture tables kb_create derived, grouped by body, and
the numpy restatement (tests/objects_ref.py) is the intended quantity: within a rounding bound of the same formulas in
float64 and, outside the objects, of the distance to a dense sampling of the outline.  BatchedKilobotsEnv checks object_obs
at construction."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from tests import objects_ref as ref
from tests.host_common import Handle, lib  # noqa: F401
from tests.sensing_common import f32, kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, 'include', 'kilobots_hip.h')).read()
    assert re.search(r'\bint\s+kb_sense_objects\s*\(', hdr) and re.search(r'\bint\s+kb_get_outline\s*\(', hdr)
    assert re.search(r'\}\s*kb_outline\s*;', hdr)
    for name, nargs in (('kb_sense_objects', 4), ('kb_get_outline', 2)):
        assert name in nat.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == nargs
    assert set(re.findall(r'\b(kb_[a-z_]+)\s*\(', hdr)) == set(nat.EXPORTS)
    # the ctypes image of kb_outline: two counts, the arena, four per-fixture tables of 8, the vertices
    assert C.sizeof(nat.KbOutline) == 4 * (2 + 4 + 4 * nat.MAX_OBJECTS + 2 * nat.MAX_POLY_VERTS * nat.MAX_OBJECTS)
    assert [n for n, _ in nat.KbOutline._fields_] == ['num_objects', 'num_fixtures', 'arena', 'body', 'kind', 'nverts', 'radius', 'verts']


def test_validation_on_an_unbound_handle(lib):
    """Nothing here launches: the pointers are never dereferenced on the host (any aligned non-NULL value will do)."""
    obj, wall = C.c_void_p(0x1000), C.c_void_p(0x2000)
    with Handle(lib) as plain, Handle(lib, num_objects=2) as two:
        bad = [
            ('NULL sim', (None, obj, wall, None)),
            ('NULL sim, walls only', (None, None, wall, None)),
            ('both outputs NULL', (two, None, None, None)),
            ('both outputs NULL, no objects', (plain, None, None, None)),
            ('d_obj without objects', (plain, obj, wall, None)),
            ('d_obj alone without objects', (plain, obj, None, None)),
        ]
        for what, args in bad:
            lib.kb_sense_neighbors(None, 0.07, 8, obj, obj, wall, None)     # (leaves a message that the next call must replace)
            assert lib.kb_sense_objects(*args) == nat.KB_EINVAL, what
            msg = lib.kb_last_error()
            assert msg and b'kb_sense_objects' in msg, what
        # legal arguments reach the bound check
        for h, args in ((two, (obj, wall)), (two, (obj, None)), (two, (None, wall)), (plain, (None, wall))):
            assert lib.kb_sense_objects(h, *args, None) == nat.KB_ENOTBOUND
            assert b'kb_sense_objects' in lib.kb_last_error() and b'kb_bind' in lib.kb_last_error()
        # kb_get_outline needs neither buffers nor a device, but its arguments
        o = nat.KbOutline()
        assert lib.kb_get_outline(None, C.byref(o)) == nat.KB_EINVAL and b'kb_get_outline' in lib.kb_last_error()
        assert lib.kb_get_outline(two, None) == nat.KB_EINVAL
        assert lib.kb_get_outline(two, C.byref(o)) == nat.KB_OK and o.num_objects == 2


def test_kernel_uses_no_scratch_and_spills_nothing(lib):
    """The running best and the inside flag stay in registers and the tables in LDS: every instantiation has a zero private
    segment and zero spill counts in the metadata of the code object that was linked."""
    found = kernel_metadata('kb_objects_kernel')
    assert len(found) >= 1, 'no kb_objects_kernel in the code object'
    for name, fields in found:
        for key in ('.private_segment_fixed_size', '.sgpr_spill_count', '.vgpr_spill_count'):
            assert fields[key] == 0, (name, key, fields[key])


def test_outline_of_a_circle(lib):
    with Handle(lib, num_objects=1, obj_radius=[0.075]) as h:
        o = nat.outline(h)
    assert (o.num_objects, o.num_fixtures) == (1, 1)
    assert (o.body[0], o.kind[0], o.nverts[0]) == (0, nat.SHAPE_CIRCLE, 0)
    assert f32(o.radius[0]) == f32(0.075) * f32(25.0)
    assert not np.array(o.verts).any()


def test_outline_of_a_box(lib):
    w, h_ = 0.15, 0.1
    with Handle(lib, num_objects=2, obj_shape=[nat.SHAPE_CIRCLE, nat.SHAPE_BOX], obj_verts=[[[0.0, 0.0]], ref.box(w, h_)]) as h:
        o = nat.outline(h)
    assert (o.num_objects, o.num_fixtures) == (2, 2) and list(o.body)[:2] == [0, 1]
    assert (o.kind[1], o.nverts[1], o.radius[1]) == (nat.SHAPE_BOX, 4, 0.0)
    hx, hy = f32(w / 2 * 25.0), f32(h_ / 2 * 25.0)
    assert np.array_equal(f32(o.verts[1]), f32([[-hx, -hy], [hx, -hy], [hx, hy], [-hx, hy]]))      # b2PolygonShape::SetAsBox


def test_outline_of_polygons_is_the_config_bit_for_bit(lib):
    tri, quad = [[-1.3, -0.7], [1.9, -1.1], [0.1, 2.3]], [[-2.1, -1.3], [2.3, -1.7], [1.9, 1.1], [-1.1, 1.9]]
    kw = ref.fixtures_kw(2, [(nat.SHAPE_POLYGON, tri, 0, 0.0), (nat.SHAPE_POLYGON, quad, 1, 0.0)])
    with Handle(lib, **kw) as h:
        o = nat.outline(h)
    assert (o.num_objects, o.num_fixtures) == (2, 2)
    assert list(o.nverts)[:2] == [3, 4] and list(o.kind)[:2] == [nat.SHAPE_POLYGON] * 2 and list(o.radius)[:2] == [0.0, 0.0]
    assert np.array_equal(ref.bits(f32(o.verts[0])[:3]), ref.bits(f32(tri)))
    assert np.array_equal(ref.bits(f32(o.verts[1])), ref.bits(f32(quad)))
    assert not f32(o.verts[0])[3].any()


def test_outline_of_the_forms_is_grouped_by_body(lib):
    """LForm + TForm + CForm + a disc, 7 + 1 fixtures declared interleaved: they come back grouped by body, within a body in
    the order of the declaration; the arena is that of the default 2 m x 1.5 m world."""
    kw = ref.forms_kw()
    assert kw['obj_fixture_body'] == [2, 0, 1, 3, 2, 1, 0, 2]
    with Handle(lib, **kw) as h:
        o = nat.outline(h)
    assert (o.num_objects, o.num_fixtures) == (4, 8)
    assert list(o.body) == [0, 0, 1, 1, 2, 2, 2, 3]
    assert ref.FORMS_ORDER == sorted(range(8), key=lambda f: kw['obj_fixture_body'][f])     # (sorted is stable)
    for g, f in enumerate(ref.FORMS_ORDER):
        assert o.kind[g] == kw['obj_shape'][f] and o.nverts[g] == kw['obj_nverts'][f], g
        if kw['obj_shape'][f] == nat.SHAPE_CIRCLE:
            assert f32(o.radius[g]) == f32(kw['obj_radius'][f]) * f32(25.0)
        else:
            assert o.radius[g] == 0.0
            assert np.array_equal(ref.bits(f32(o.verts[g])[:o.nverts[g]]), ref.bits(f32(kw['obj_verts'][f])))
    assert list(o.arena) == [-25.0, 25.0, -18.75, 18.75]
    tab = ref.tables(o)
    assert tab['M'] == 4 and [fx['body'] for fx in tab['fixtures']] == list(o.body)


# ---- the restatement is the intended quantity -----------------------------------------------------------------------------
OBJ_XY = f32([[12.5, 8.75], [-12.5, 8.75], [-12.5, -8.75], [12.5, -8.75]])      # world units
OBJ_TH = f32([0.4, -2.1, 1.2, 0.8])


def to_world(local, m):
    c, s = np.cos(np.float64(OBJ_TH[m])), np.sin(np.float64(OBJ_TH[m]))
    return np.stack([c * local[:, 0] - s * local[:, 1], s * local[:, 0] + c * local[:, 1]], -1) + OBJ_XY[m].astype(np.float64)


@pytest.fixture(scope='module')
def forms(lib):
    """The forms scene with 200 kilobots around each of the four shapes and 50 placed inside each: the outline's tables, the
    float32 state, the restatement in float32 and in float64, and which shape every kilobot was drawn for."""
    with Handle(lib, **ref.forms_kw()) as h:
        tab = ref.tables(nat.outline(h))
    rng = np.random.RandomState(11)
    pts, owner, placed = [], [], []
    for m in range(4):
        pts.append(OBJ_XY[m] + rng.normal(scale=4.0, size=(200, 2)))
        fx = [f for f in tab['fixtures'] if f['body'] == m]
        inner = []
        for j in range(50):
            f = fx[j % len(fx)]
            if f['n'] == 0:
                rad, ang = float(f['radius']) * np.sqrt(rng.uniform(0.25, 0.9)), rng.uniform(-np.pi, np.pi)
                inner.append([rad * np.cos(ang), rad * np.sin(ang)])
            else:
                wgt = rng.dirichlet(np.full(f['n'], 2.0))
                inner.append(wgt @ f['verts'].astype(np.float64))
        pts.append(to_world(np.array(inner), m))
        owner += [m] * 250
        placed += [False] * 200 + [True] * 50
    xy = f32(np.concatenate(pts))
    th = f32(rng.uniform(-np.pi, np.pi, size=len(xy)))
    assert np.abs(xy).max() <= 32.0
    state = (xy[:, 0].copy(), xy[:, 1].copy(), th, OBJ_XY[:, 0].copy(), OBJ_XY[:, 1].copy(), OBJ_TH)
    return dict(tab=tab, state=state, owner=np.array(owner), placed=np.array(placed),
                r32=ref.restate_env(tab, *state), r64=ref.restate_env(tab, *state, ft=np.float64))


def test_restatement_is_within_the_rounding_bound_of_float64(forms):
    """The float32 restatement against the same formulas in float64, bound ref.BOUND_M = 1.95e-5 m (derived in
    tests/objects_ref.py from the operation count and coordinates of at most 32 world units).  The distance is continuous and is compared
    everywhere.  The point is not: where two candidates are nearly as close, the two evaluations may pick different ones.
    There, and only there, the vectors may differ by more than the bound, and then the float64 evaluation itself must show
    the near tie (its two best candidates within 2 bounds of each other).  The inside flag may differ only on the boundary,
    where the float64 distance is within the bound."""
    o32, w32, a32 = forms['r32']
    o64, w64, a64 = forms['r64']
    assert o32.dtype == np.float32 and o64.dtype == np.float64
    placed, owner = forms['placed'], forms['owner']
    own = np.arange(len(owner)), owner
    assert o64[own][placed, 3].sum() == placed.sum()                   # every placed kilobot is inside its shape
    assert (o64[..., 3].sum(0) >= 50).all() and (o64[own][~placed, 3] == 0).sum() > 400
    derr = np.abs(o32[..., 2] - o64[..., 2])
    verr = np.abs(o32[..., :2] - o64[..., :2]).max(-1)
    werr = np.abs(w32[:, :3] - w64[:, :3]).max(-1)
    print('largest errors in metres: distance %.3g, point %.3g, wall %.3g; bound %.3g' % (derr.max(), verr.max(), werr.max(), ref.BOUND_M))
    assert (derr <= ref.BOUND_M).all()
    assert (werr <= ref.BOUND_M).all() and np.array_equal(w32[:, 3], w64[:, 3])
    far = verr > ref.BOUND_M
    margin = a64['second'] - o64[..., 2] * 25.0
    print('%d of %d points differ by more than the bound, all of them near ties: largest margin %.3g world units'
          % (far.sum(), far.size, margin[far].max(initial=0.0)))
    assert (a32['winner'][far] != a64['winner'][far]).all() and (margin[far] <= 2 * ref.BOUND_WU).all()
    assert far.sum() < 0.01 * far.size
    flip = o32[..., 3] != o64[..., 3]
    assert (o64[..., 2][flip] <= ref.BOUND_M).all() and flip.sum() < 0.01 * flip.size
    assert derr.max() > 0       # (the bound is not met trivially)


def test_distance_outside_equals_a_dense_sampling_of_the_outline(forms):
    """For kilobots outside every fixture of an object the distance is the distance to the object's outline: the minimum over
    2000 points per fixture edge (per circle) in float64.  A sampled minimum is never below the true distance and at most
    half a sample spacing above it (the nearest point of the outline has a sample within half a spacing along its edge), so
    sampled - spacing / 2 - bound <= distance <= sampled + bound, with the rounding bound of the test above."""
    tab, (x, y, th, ox, oy, oth) = forms['tab'], forms['state']
    o32 = forms['r32'][0]
    S = 2000
    u = np.linspace(0.0, 1.0, S)
    checked = 0
    for m in range(tab['M']):
        c, s = np.cos(np.float64(oth[m])), np.sin(np.float64(oth[m]))
        dx, dy = x.astype(np.float64) - np.float64(ox[m]), y.astype(np.float64) - np.float64(oy[m])
        p = np.stack([c * dx + s * dy, c * dy - s * dx], -1)
        sampled, spacing = np.full(len(p), np.inf), 0.0
        for fx in tab['fixtures']:
            if fx['body'] != m:
                continue
            if fx['n'] == 0:
                ang = 2 * np.pi * np.arange(S) / S
                pts = float(fx['radius']) * np.stack([np.cos(ang), np.sin(ang)], -1)
                spacing = max(spacing, 2 * np.pi * float(fx['radius']) / S)
                sampled = np.minimum(sampled, np.sqrt(((p[:, None] - pts[None]) ** 2).sum(-1)).min(1))
                continue
            v = fx['verts'].astype(np.float64)
            for k in range(fx['n']):
                a, b = v[k], v[(k + 1) % fx['n']]
                pts = a + u[:, None] * (b - a)
                spacing = max(spacing, np.linalg.norm(b - a) / (S - 1))
                sampled = np.minimum(sampled, np.sqrt(((p[:, None] - pts[None]) ** 2).sum(-1)).min(1))
        outside = o32[:, m, 3] == 0
        d = o32[:, m, 2].astype(np.float64) * 25.0
        print('object %d: %d outside, spacing %.3g, distance - sampled in [%.3g, %.3g] world units'
              % (m, outside.sum(), spacing, (d - sampled)[outside].min(), (d - sampled)[outside].max()))
        assert outside.sum() > 600
        assert (d[outside] <= sampled[outside] + ref.BOUND_WU).all()
        assert (d[outside] >= sampled[outside] - spacing / 2 - ref.BOUND_WU).all()
        checked += outside.sum()
    assert checked > 3000


def test_ties_go_to_the_earlier_candidate_on_the_restatement():
    """On the diagonal of an axis-aligned square the bottom and the right edge (edges 0 and 1 of SetAsBox) are equally far:
    edge 0 wins, and the point is straight below."""
    tab = dict(M=1, arena=f32([-25, 25, -18.75, 18.75]),
               fixtures=[dict(body=0, kind=1, n=4, radius=np.float32(0), verts=f32([[-2, -2], [2, -2], [2, 2], [-2, 2]]))])
    z = f32([0.0])
    obj, wall, aux = ref.restate_env(tab, f32([1.0]), f32([-1.0]), z, z, z, z)
    assert aux['ties'][0, 0] == 2 and aux['winner'][0, 0] == 0
    assert obj[0, 0].tolist() == [0.0, f32(-1.0) / f32(25.0), f32(1.0) / f32(25.0), 1.0]
    # at the origin walls 0 and 1 are equally far, walls 2 and 3 are nearer and equally far: 2 wins
    _, wall, aux = ref.restate_env(tab, z, z, z, z, z, z)
    assert wall[0].tolist() == [0.0, f32(-18.75) / f32(25.0), f32(18.75) / f32(25.0), 2.0] and aux['walltie'][0] == 2


def test_batched_env_object_obs_without_a_gpu():
    import torch
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    from tests.oracle_backend import OracleBackend
    env = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3)
    env.reset()
    a = torch.zeros(3, 16, 2)
    a[..., 0] = 0.01
    assert env.step(a)[3] == {}
    assert env.object_obs is False
    with pytest.raises(ValueError):
        env.object_points()
    for bad in (0.5, 'yes', (True,), 2):
        with pytest.raises(ValueError):
            BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, object_obs=bad)
    for off in (None, False):
        same = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3, object_obs=off)
        assert same.object_obs is False and torch.equal(same.reset(), BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3).reset())
        assert same.step(a)[3] == {}
    ok = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3, object_obs=True)
    assert ok.object_obs is True
    assert torch.equal(ok.reset(), BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3).reset())
