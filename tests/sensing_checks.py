"""The comparers of the sensing suites that more than one test module uses: each calls a KilobotSim sensing method,
synchronises, and compares every word of the result with the numpy restatement of the kernel's definition (tests/*_ref.py)
on the state of the sim as it is on the device.  Everything is compared for equality; no tolerances."""
import numpy as np
import torch

from gym_kilobots_amd import _native as nat
from oracle import oracle as O
from tests import clusters_ref
from tests import contacts_ref
from tests import contacts_scenes
from tests import coverage_ref
from tests import histogram_ref
from tests import objects_ref
from tests import reduce_ref
from tests import render_ref
from tests import targets_ref
from tests.gpu_common import cpu, dev, state


def differing(t, w):
    """Elements of a device tensor whose bits differ from the array's."""
    a = cpu(t)
    assert a.dtype == w.dtype and a.shape == w.shape, (a.dtype, w.dtype, a.shape, w.shape)
    return a.view(np.uint32) != w.view(np.uint32)


# ---- kb_sense_neighbors ------------------------------------------------------------------------------------------------------
def restate_neighbors(x, y, th, R, k):
    """The definition, brute force.  x, y [E, N] float32 world units, th [E, N] float32.
    Returns (index [E, N, k] int32, rel [E, N, k, 4] float32, count [E, N] uint32, zero-distance neighbours [E, N])."""
    assert x.dtype == y.dtype == th.dtype == np.float32, 'the poses are %s, %s, %s, not float32' % (x.dtype, y.dtype, th.dtype)
    E, N = x.shape
    W = np.float32(25)
    Rw = np.float32(R) * W
    R2 = Rw * Rw
    index = np.full((E, N, k), -1, np.int32)
    rel = np.zeros((E, N, k, 4), np.float32)
    count = np.zeros((E, N), np.uint32)
    zeros = np.zeros((E, N), np.int64)
    for e in range(E):
        ex = x[e][None, :] - x[e][:, None]          # [i, j] = x_j - x_i
        ey = y[e][None, :] - y[e][:, None]
        d2 = ex * ex + ey * ey
        assert ex.dtype == d2.dtype == np.float32, 'the offsets are %s and their squares %s, not float32' % (ex.dtype, d2.dtype)
        inr = ~(d2 > R2)
        np.fill_diagonal(inr, False)
        count[e] = inr.sum(1)
        zeros[e] = (inr & (d2 == 0)).sum(1)
        for i in range(N):
            js = np.nonzero(inr[i])[0]
            js = js[np.lexsort((js, d2[i, js]))][:k]
            m = len(js)
            s, c = (np.float32(v) for v in O.sincosf(float(th[e, i])))
            exi, eyi = ex[i, js], ey[i, js]
            index[e, i, :m] = js
            rel[e, i, :m, 0] = (c * exi + s * eyi) / W
            rel[e, i, :m, 1] = (c * eyi - s * exi) / W
            rel[e, i, :m, 2] = np.sqrt(d2[i, js]) / W
            rel[e, i, :m, 3] = th[e, js] - th[e, i]
    return index, rel, count, zeros


def check_neighbors(g, R, k, what=''):
    """Items 3-5 of the sweep: values, count == sense(R), padding."""
    idx, rel, cnt = g.neighbors(R, k)
    sensed = g.sense(R)
    torch.cuda.synchronize()
    assert idx.dtype == torch.int32 and rel.dtype == torch.float32 and cnt.dtype == torch.int32, \
        '%s: dtypes %s, %s, %s' % (what, idx.dtype, rel.dtype, cnt.dtype)
    E, N = g.num_envs, g.num_bots
    assert tuple(idx.shape) == (E, N, k) and tuple(rel.shape) == (E, N, k, 4) and tuple(cnt.shape) == (E, N), \
        '%s: shapes %s, %s, %s' % (what, tuple(idx.shape), tuple(rel.shape), tuple(cnt.shape))
    idx, rel, cnt = cpu(idx), cpu(rel), cpu(cnt).view(np.uint32)
    widx, wrel, wcnt, zeros = restate_neighbors(*state(g), R, k)
    bad = np.argwhere(idx != widx)
    print('%s E=%d N=%d R=%g k=%d: %d index mismatches, %d rel words differ, %d counts differ, max count %d'
          % (what, E, N, R, k, len(bad), int((rel.view(np.uint32) != wrel.view(np.uint32)).sum()), int((cnt != wcnt).sum()), int(wcnt.max())))
    assert np.array_equal(cnt, wcnt), what
    assert np.array_equal(cnt, cpu(sensed).view(np.uint32)), what
    assert np.array_equal(idx, widx), (what, bad[:5])
    assert np.array_equal(rel.view(np.uint32), wrel.view(np.uint32)), what
    pad = np.arange(k)[None, None, :] >= np.minimum(cnt, k)[..., None]
    assert (idx[pad] == -1).all() and (rel.view(np.uint32)[pad] == 0).all(), what
    assert (idx[~pad] >= 0).all() and (idx[~pad] < N).all(), '%s: a listed index outside 0 .. %d' % (what, N - 1)
    return idx, rel, cnt, zeros


# ---- kb_sense_histogram ------------------------------------------------------------------------------------------------------
def check_histogram(g, R, rings, sectors, what=''):
    """hist equals the restatement; its rows sum to count, which is what sense(R) gives."""
    hist, cnt = g.neighbor_histogram(R, rings, sectors, count=True)
    sensed = g.sense(R)
    torch.cuda.synchronize()
    E, N = g.num_envs, g.num_bots
    assert hist.dtype == torch.float32 and cnt.dtype == torch.int32, '%s: dtypes %s, %s' % (what, hist.dtype, cnt.dtype)
    assert tuple(hist.shape) == (E, N, rings, sectors) and tuple(cnt.shape) == (E, N), \
        '%s: shapes %s, %s' % (what, tuple(hist.shape), tuple(cnt.shape))
    hist, cnt = cpu(hist), cpu(cnt).view(np.uint32)
    want, wcnt = histogram_ref.restate(*state(g), R, rings, sectors)
    print('%s E=%d N=%d R=%g grid=%dx%d: %d of %d bins differ, %d counts differ, max count %d, bins hit %d of %d'
          % (what, E, N, R, rings, sectors, int((hist != want).sum()), hist.size, int((cnt != wcnt).sum()), int(wcnt.max()),
             int((want.sum((0, 1)) > 0).sum()), rings * sectors))
    assert np.array_equal(cnt, wcnt), what
    assert np.array_equal(cnt, cpu(sensed).view(np.uint32)), what
    assert np.array_equal(hist, want), (what, np.argwhere(hist != want)[:5])
    assert np.array_equal(hist.sum((2, 3)), cnt.astype(np.float32)), what
    return hist, cnt


# ---- kb_sense_reduce ---------------------------------------------------------------------------------------------------------
def check_reduce(g, inr, R, op, values, scale=65536.0, what=''):
    """neighbor_reduce equals the restatement bit for bit; its count is what sense(R) gives.  values: numpy [E, N(, C)]."""
    v = dev(values)
    out, cnt = g.neighbor_reduce(v, R, op=op, scale=scale, count=True)
    sensed = g.sense(R)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and cnt.dtype == torch.int32, '%s: dtypes %s, %s' % (what, out.dtype, cnt.dtype)
    assert tuple(out.shape) == values.shape and tuple(cnt.shape) == values.shape[:2], \
        '%s: shapes %s, %s for messages of %s' % (what, tuple(out.shape), tuple(cnt.shape), values.shape)
    assert torch.equal(v.view(torch.int32), dev(values).view(torch.int32)), \
        '%s: the messages were changed' % what          # out of place: the messages are untouched
    out, cnt = cpu(out), cpu(cnt).view(np.uint32)
    envs = [reduce_ref.reduce_env(inr[e], values[e], op, scale) for e in range(g.num_envs)]
    want, wcnt = np.stack([o for o, _ in envs]), np.stack([c for _, c in envs])
    differ = reduce_ref.bits(out) != reduce_ref.bits(want)
    print('%s E=%d N=%d R=%g op=%s shape=%s scale=%g: %d of %d words differ, %d counts differ, at most %d heard'
          % (what, g.num_envs, g.num_bots, R, op, values.shape[2:], scale, int(differ.sum()), out.size, int((cnt != wcnt).sum()), int(wcnt.max())))
    assert np.array_equal(cnt, wcnt), what
    assert np.array_equal(cnt, cpu(sensed).view(np.uint32)), what
    assert not differ.any(), (what, op, np.argwhere(differ)[:5])
    return out, cnt


def messages(E, N, C, seed):
    return np.random.RandomState(seed).uniform(-4.0, 4.0, size=(E, N, C) if C else (E, N)).astype(np.float32)


# ---- kb_render ---------------------------------------------------------------------------------------------------------------
def render_scene_of(g):
    """What the restatement needs of a sim, as it is on the device: keywords of render_ref.restate."""
    torch.cuda.synchronize()
    E = g.num_envs
    kw = dict(bot_radius=g.cfg.bot_radius, x=cpu(g.x), y=cpu(g.y), th=cpu(g.theta))
    if g.num_objects:
        kw.update(ox=cpu(g.ox), oy=cpu(g.oy), oth=cpu(g.otheta))
    if g.light_type in (nat.LIGHT_CIRCULAR, nat.LIGHT_MOMENTUM):
        kw['lights'] = ([g.cfg.light_radius], cpu(g.light_x).reshape(E, 1), cpu(g.light_y).reshape(E, 1))
    elif g.light_type == nat.LIGHT_COMPOSITE:
        n = g.cfg.light_count
        kw['lights'] = (list(g.cfg.lightc_radius)[:n], cpu(g.light_x).reshape(E, n), cpu(g.light_y).reshape(E, n))
    return kw


def want_render(g, width, height, layers=render_ref.ALL, style=None, body=None, mark=None):
    return render_ref.restate(objects_ref.tables(g.outline()), width, height, layers, style=style, body=body, mark=mark, **render_scene_of(g))


def colour_words(t):
    return None if t is None else dev(np.ascontiguousarray(t, dtype=np.int64).astype(np.int32))


def check_render(g, width, height, layers=render_ref.ALL, style=None, body=None, mark=None, what='', w=None):
    w = want_render(g, width, height, layers, style, body, mark) if w is None else w
    got = g.render(width, height, layers, style=style, body_rgb=colour_words(body), mark_rgb=colour_words(mark))
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == w.shape == (g.num_envs, height, width, 3) and got.is_contiguous(), \
        '%s: a frame of %s %s (contiguous: %s), the restatement has %s' % (what, got.dtype, tuple(got.shape), got.is_contiguous(), w.shape)
    d = cpu(got) != w
    print('%s E=%d N=%d %d x %d layers %d: %d of %d bytes differ' % (what, g.num_envs, g.num_bots, width, height, layers, int(d.sum()), d.size))
    assert not d.any(), (what, width, height, layers, np.argwhere(d)[:5])
    return w


# ---- kb_sense_clusters -------------------------------------------------------------------------------------------------------
CLUSTERS_NAMES = ('label', 'size', 'table', 'stats')
CLUSTERS_DTYPES = (torch.int32, torch.int32, torch.float32, torch.int32)


def float_bits(a):
    """The bit patterns of a float32 array; an integer array as it is."""
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def restate_clusters(g, inr, select=None):
    x, y = state(g)[:2]
    envs = [clusters_ref.clusters_env(inr[e], x[e], y[e], None if select is None else select[e]) for e in range(len(inr))]
    return tuple(np.stack([env[k] for env in envs]) for k in range(4))


def check_clusters(g, inr, R, select=None, what=''):
    """clusters() with all four outputs equals the restatement.  select: numpy [E, N] bool or uint8, or None.  Returns the
    restatement."""
    s = None if select is None else dev(select)
    got = g.clusters(R, select=s, size=True, table=True, stats=True)
    torch.cuda.synchronize()
    want = restate_clusters(g, inr, select)
    assert s is None or torch.equal(s, dev(select)), '%s: the selection was changed' % what
    for name, dtype, t, w in zip(CLUSTERS_NAMES, CLUSTERS_DTYPES, got, want):
        assert t.dtype == dtype and tuple(t.shape) == w.shape, name
        differ = float_bits(cpu(t)) != float_bits(w)
        print('%s E=%d N=%d R=%g select=%s %s: %d of %d words differ' % (what, g.num_envs, g.num_bots, R, select is not None, name, int(differ.sum()), w.size))
        assert not differ.any(), (what, name, np.argwhere(differ)[:5])
    return want


# ---- kb_sense_coverage -------------------------------------------------------------------------------------------------------
COVERAGE_PARTS = ('owner', 'dist', 'cells', 'stats')


def want_coverage(g, gw, gh, sel=None):
    """The restatement on the state of the sim as it is on the device."""
    torch.cuda.synchronize()
    return coverage_ref.restate(objects_ref.tables(g.outline()), gw, gh, cpu(g.x), cpu(g.y), cpu(g.theta), None if sel is None else cpu(sel))


def check_coverage(g, gw, gh, sel=None, what='', w=None, alone=True):
    """All four outputs in one call, then each alone with the others NULL, against the restatement w."""
    PARTS = COVERAGE_PARTS
    w = want_coverage(g, gw, gh, sel) if w is None else w
    got = g.coverage(gw, gh, select=sel)
    torch.cuda.synchronize()
    assert got._fields == PARTS and got.owner.dtype == torch.int32 and all(t.is_contiguous() for t in got), \
        '%s: fields %s, owner of %s, contiguous %s' % (what, got._fields, got.owner.dtype, [t.is_contiguous() for t in got])
    for name in PARTS:
        d = differing(getattr(got, name), getattr(w, name))
        print('%s E=%d N=%d %d x %d %s: %d of %d words differ' % (what, g.num_envs, g.num_bots, gw, gh, name, int(d.sum()), d.size))
        assert not d.any(), (what, gw, gh, name, np.argwhere(d)[:5])
    if alone:
        for name in PARTS:
            part = g.coverage(gw, gh, select=sel, **{n: n == name for n in PARTS})
            torch.cuda.synchronize()
            assert [t is None for t in part] == [n != name for n in PARTS], \
                '%s: asked for %s alone, got %s' % (what, name, [n for n, t in zip(PARTS, part) if t is not None])
            assert not differing(getattr(part, name), getattr(w, name)).any(), (what, gw, gh, name, 'alone')
    return w


# ---- kb_sense_targets --------------------------------------------------------------------------------------------------------
TARGETS_PARTS = ('index', 'rel', 'owner', 'dist', 'stats')


def want_targets(g, points, tol, bot_select=None, slot_select=None):
    """The restatement on the state of the sim as it is on the device."""
    torch.cuda.synchronize()
    host = lambda t: None if t is None else cpu(t.to(torch.uint8))
    return targets_ref.restate(cpu(g.x), cpu(g.y), cpu(g.theta), cpu(points), tol, host(bot_select), host(slot_select))


def check_targets(g, points, tol, what='', w=None, alone=True, **sel):
    """All five outputs in one call, then each alone with the others NULL, against the restatement w."""
    PARTS = TARGETS_PARTS
    w = want_targets(g, points, tol, **sel) if w is None else w
    got = g.targets(points, tol, **sel)
    torch.cuda.synchronize()
    assert got._fields == PARTS and got.index.dtype == got.owner.dtype == torch.int32 and all(t.is_contiguous() for t in got), \
        '%s: fields %s, index of %s, owner of %s, contiguous %s' % (what, got._fields, got.index.dtype, got.owner.dtype, [t.is_contiguous() for t in got])
    for name in PARTS:
        d = differing(getattr(got, name), getattr(w, name))
        print('%s E=%d N=%d K=%d %s: %d of %d words differ' % (what, g.num_envs, g.num_bots, points.shape[-2], name, int(d.sum()), d.size))
        assert not d.any(), (what, name, np.argwhere(d)[:5])
    if alone:
        for name in PARTS:
            part = g.targets(points, tol, **sel, **{n: n == name for n in PARTS})
            torch.cuda.synchronize()
            assert [t is None for t in part] == [n != name for n in PARTS], \
                '%s: asked for %s alone, got %s' % (what, name, [n for n, t in zip(PARTS, part) if t is not None])
            assert not differing(getattr(part, name), getattr(w, name)).any(), (what, name, 'alone')
    return w


# ---- kb_sense_contacts -------------------------------------------------------------------------------------------------------
def want_contacts(g, k, scale=65536.0):
    torch.cuda.synchronize()
    return contacts_ref.contacts_ref(cpu(g.ws_cnt), cpu(g.ws_key), cpu(g.ws_acc), g.contact_capacity, g.num_bots, g.num_objects,
                                     contacts_scenes.fixture_body(g.cfg), k, scale)


def same_contacts(got, exp, what=''):
    """The four outputs against the restatement: partner by equality, the floats by bit pattern, None where None."""
    torch.cuda.synchronize()
    for name, a, b in zip(('partner', 'impulse', 'touch', 'obj'), got, exp):
        assert (a is None) == (b is None), (what, name)
        if a is None:
            continue
        a = cpu(a)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape)
        ia, ib = a.view(np.int32), b.view(np.int32)
        assert np.array_equal(ia, ib), '%s: %s differs in %d of %d words, first at %s' % (what, name, (ia != ib).sum(), ia.size, np.argwhere(ia != ib)[0])
