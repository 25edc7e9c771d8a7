"""Numpy restatement of kb_render's definition (include/kilobots_hip.h), shared by the render tests.

Brute force: every pixel meets every kilobot of its env, in index order, and the last one that covers it wins.  float32
arrays wherever the definition rounds in fp32, so every operation rounds on its own like the kernel's (-ffp-contract=off);
the blend is integer arithmetic.  The arena and the fixtures come ONLY from kb_get_outline (objects_ref.tables), sine and
cosine are the oracle library's sincosf (objects_ref.sincos), and the object layer is the inside flag of
objects_ref.restate_env for kilobots placed on the pixel centres, as grid_ref.object_masks takes it: the predicate is not
restated a second time.  Comparisons with the device are by equality of the bytes."""
import numpy as np

from tests import objects_ref

OBJECTS, BOTS, LIGHT = 1, 2, 4
ALL = OBJECTS | BOTS | LIGHT
f32 = np.float32
S = f32(25.0)
DEFAULT_STYLE = dict(table=(255, 255, 255), body=(150, 150, 150), ring=(100, 100, 100), mark=(255, 255, 255), light=(255, 255, 30),
                     light_alpha=150, obj=[(93, 133, 195)] * 8)


def style_of(overrides=None):
    st = dict(DEFAULT_STYLE)
    st['obj'] = list(st['obj'])
    for k, v in dict(overrides or {}).items():
        if k == 'obj':
            st['obj'][:len(v)] = [tuple(c) for c in v]
        else:
            st[k] = v
    return st


def constants(tab, bot_radius, width, height):
    """The host constants as float32, one operation each: dict(xmin, ymin, cw, ch, Ro, Ro2, Ri, Ri2, Lf, Hw)."""
    xmin, xmax, ymin, ymax = tab['arena']
    assert tab['arena'].dtype == np.float32
    r = f32(bot_radius)
    ro = r + f32(0.002)
    Ro = ro * S
    Ri = (ro - f32(0.005)) * S
    c = dict(xmin=xmin, ymin=ymin, cw=(xmax - xmin) / f32(width), ch=(ymax - ymin) / f32(height), Ro=Ro, Ro2=Ro * Ro, Ri=Ri, Ri2=Ri * Ri,
             Lf=(r - f32(0.005)) * S, Hw=f32(0.0025) * S)
    assert all(v.dtype == np.float32 for v in c.values())
    return c


def centres(tab, bot_radius, width, height):
    """(px [width], py [height]) float32: the pixel centres by column and by row (row 0 at ymax)."""
    c = constants(tab, bot_radius, width, height)
    px = c['xmin'] + (np.arange(width).astype(np.float32) + f32(0.5)) * c['cw']
    py = c['ymin'] + ((height - 1 - np.arange(height)).astype(np.float32) + f32(0.5)) * c['ch']
    assert px.dtype == py.dtype == np.float32
    return px, py


def words(rgb):
    """0x00RRGGBB words -> [..., 3] uint8."""
    w = np.asarray(rgb).astype(np.int64) & 0xFFFFFFFF
    return np.stack([(w >> 16) & 255, (w >> 8) & 255, w & 255], -1).astype(np.uint8)


def object_flags(tab, px, py, ox, oy, oth):
    """[M, height, width] bool: the inside flag of objects_ref.restate_env at every pixel centre.  Only the pixels within the
    bounding circle of an object (its farthest vertex or its radius, plus a world unit) are handed to it: no point outside
    that circle is inside a fixture, and the margin is five orders of magnitude above any rounding here."""
    H, W = len(py), len(px)
    X, Y = np.tile(px, H), np.repeat(py, W)
    flags = np.zeros((tab['M'], H * W), dtype=bool)
    for m in range(tab['M']):
        reach = max([float(np.sqrt((fx['verts'].astype(np.float64) ** 2).sum(-1).max())) if fx['n'] else float(fx['radius'])
                     for fx in tab['fixtures'] if fx['body'] == m]) + 1.0
        near = np.flatnonzero((X.astype(np.float64) - float(ox[m])) ** 2 + (Y.astype(np.float64) - float(oy[m])) ** 2 <= reach * reach)
        if len(near):
            obj = objects_ref.restate_env(tab, X[near], Y[near], np.zeros(len(near), dtype=np.float32), ox, oy, oth)[0]
            flags[m, near] = obj[:, m, 3] == 1
    return flags.reshape(tab['M'], H, W)


def bot_layer(c, px, py, x, y, th):
    """(win [H, W] int: the highest covering kilobot or -1; kind [H, W] int: 0 body, 1 ring, 2 mark where win >= 0)."""
    H, W = len(py), len(px)
    win = np.full((H, W), -1)
    kind = np.zeros((H, W), dtype=int)
    sn, cs = objects_ref.sincos(th, np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for b in range(len(x)):
            qx = px - x[b]
            qy = py - y[b]
            dd = (qx * qx)[None, :] + (qy * qy)[:, None]
            assert dd.dtype == np.float32
            cover = dd <= c['Ro2']
            if not cover.any():
                continue
            a = (cs[b] * qx)[None, :] + (sn[b] * qy)[:, None]
            l = (cs[b] * qy)[:, None] - (sn[b] * qx)[None, :]
            assert a.dtype == l.dtype == np.float32
            mark = (c['Lf'] > 0) & (a >= 0) & (a <= c['Lf']) & (np.abs(l) <= c['Hw'])
            ring = ~(c['Ri'] > 0) | (dd > c['Ri2'])
            k = np.where(mark, 2, np.where(ring, 1, 0))
            win = np.where(cover, b, win)
            kind = np.where(cover, k, kind)
    return win, kind


def restate_env(tab, width, height, layers, bot_radius, x, y, th, ox=None, oy=None, oth=None, lights=None, style=None, body=None, mark=None, rows=None):
    """One env: x, y, th [N] float32 (world units, radians); ox, oy, oth [M] float32; lights = (radii [L] in metres, lx [L], ly
    [L] float32 in metres) of the positional components or None; body, mark [N] 0x00RRGGBB words or None -> [height, width, 3]
    uint8.  rows: the rows of the frame to restate (an index array), for frames too large to restate whole -> [len(rows),
    width, 3]."""
    for v in (x, y, th):
        assert v.dtype == np.float32
    st = style_of(style)
    c = constants(tab, bot_radius, width, height)
    px, py = centres(tab, bot_radius, width, height)
    if rows is not None:
        py, height = py[rows], len(rows)
    img = np.empty((height, width, 3), dtype=np.uint8)
    img[:] = np.array(st['table'], dtype=np.uint8)
    if layers & OBJECTS and tab['M']:
        flags = object_flags(tab, px, py, ox, oy, oth)
        for m in range(tab['M']):           # painter's order: a higher object paints over a lower one
            img[flags[m]] = np.array(st['obj'][m], dtype=np.uint8)
    if layers & BOTS:
        win, kind = bot_layer(c, px, py, x, y, th)
        hit = win >= 0
        w = np.where(hit, win, 0)
        bcol = words(body)[w] if body is not None else np.broadcast_to(np.array(st['body'], dtype=np.uint8), (height, width, 3))
        mcol = words(mark)[w] if mark is not None else np.broadcast_to(np.array(st['mark'], dtype=np.uint8), (height, width, 3))
        col = np.where((kind == 2)[..., None], mcol, np.where((kind == 1)[..., None], np.array(st['ring'], dtype=np.uint8), bcol))
        img = np.where(hit[..., None], col, img).astype(np.uint8)
    if layers & LIGHT and lights is not None:
        radii, lx, ly = lights
        A = int(st['light_alpha'])
        for l in range(len(radii)):
            Rl = f32(radii[l]) * S
            Rl2 = Rl * Rl
            fx = f32(lx[l]) * S - px
            fy = f32(ly[l]) * S - py
            d = (fx * fx)[None, :] + (fy * fy)[:, None]
            assert d.dtype == np.float32
            inside = d <= Rl2
            v = img.astype(np.int64)
            blend = (np.array(st['light'], dtype=np.int64) * A + v * (255 - A) + 127) // 255
            img = np.where(inside[..., None], blend, v).astype(np.uint8)
    return img


def restate(tab, width, height, layers, bot_radius, x, y, th, ox=None, oy=None, oth=None, lights=None, style=None, body=None, mark=None):
    """x, y, th [E, N]; ox, oy, oth [E, M] or None; lights = (radii [L], lx [E, L], ly [E, L]) or None; body, mark [E, N] or
    None -> [E, height, width, 3] uint8."""
    E = x.shape[0]
    pick = lambda v, e: None if v is None else v[e]
    return np.stack([restate_env(tab, width, height, layers, bot_radius, x[e], y[e], th[e], pick(ox, e), pick(oy, e), pick(oth, e),
                                 None if lights is None else (lights[0], lights[1][e], lights[2][e]), style, pick(body, e), pick(mark, e))
                     for e in range(E)])
