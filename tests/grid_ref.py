"""Numpy restatement of kb_sense_grid's definition (include/kilobots_hip.h), shared by the occupancy-grid tests.

float32 arrays wherever the definition rounds in fp32, so every operation rounds on its own like the kernel's
(-ffp-contract=off); the sums are integer sums.  The arena and the fixtures come ONLY from kb_get_outline
(objects_ref.tables), sine and cosine are the oracle library's sincosf, the quantisation is reduce_ref.quant, and the object
planes are the inside flag of objects_ref.restate_env for kilobots placed on the cell centres: the predicate is not restated
a second time.  Comparisons with the device are by equality of the bit patterns."""
import numpy as np

from tests import objects_ref
from tests import reduce_ref

COUNT, FLOW, OBJECTS = 1, 2, 4
ALL = COUNT | FLOW | OBJECTS
SCALE = np.float32(65536.0)
f32 = np.float32


def constants(tab, gw, gh):
    """(xmin, ymin, cw, ch, icw, ich) as float32: one subtraction and one division each."""
    xmin, xmax, ymin, ymax = tab['arena']
    assert tab['arena'].dtype == np.float32
    wx, wy = xmax - xmin, ymax - ymin
    return xmin, ymin, wx / f32(gw), wy / f32(gh), f32(gw) / wx, f32(gh) / wy


def axis_cell(v, lo, inv, n):
    """Cell indices [N] int of float32 coordinates along one axis: 0 if !(t > 0), n - 1 if t >= n, else trunc(t)."""
    assert v.dtype == np.float32
    with np.errstate(invalid='ignore', over='ignore'):
        t = (v - lo) * inv
        assert t.dtype == np.float32
        low, high = ~(t > 0), t >= f32(n)
        return np.where(low, 0, np.where(high, n - 1, np.where(low | high, f32(0), t).astype(np.int64)))


def cells(tab, gw, gh, x, y):
    """(ix, iy) of the kilobots at x, y [N] float32 (world units)."""
    xmin, ymin, _, _, icw, ich = constants(tab, gw, gh)
    return axis_cell(x, xmin, icw, gw), axis_cell(y, ymin, ich, gh)


def centres(tab, gw, gh):
    """(cx, cy) [gh * gw] float32 of the cell centres, row by row."""
    xmin, ymin, cw, ch, _, _ = constants(tab, gw, gh)
    cx = xmin + (np.arange(gw).astype(np.float32) + f32(0.5)) * cw
    cy = ymin + (np.arange(gh).astype(np.float32) + f32(0.5)) * ch
    assert cx.dtype == cy.dtype == np.float32
    return np.tile(cx, gh), np.repeat(cy, gw)


def quantised_headings(th):
    """(qc, qs) int32 [N]: the fixed-point images of the cosine and the sine of float32 headings."""
    s, c = objects_ref.sincos(th, np.float32)
    return reduce_ref.quant(c, SCALE), reduce_ref.quant(s, SCALE)


def object_masks(tab, gw, gh, ox, oy, oth, ft=np.float32):
    """[M, gh, gw] of dtype ft: the inside flag of objects_ref.restate_env for a kilobot on every cell centre; with
    ft = float64 the same predicate on the same float32 centres in double.  Also returns the distances [M, gh, gw] to the
    outline in metres."""
    cx, cy = centres(tab, gw, gh)
    obj = objects_ref.restate_env(tab, cx, cy, np.zeros_like(cx), ox, oy, oth, ft)[0]
    return (np.ascontiguousarray(obj[:, :, 3].T).reshape(tab['M'], gh, gw), np.ascontiguousarray(obj[:, :, 2].T).reshape(tab['M'], gh, gw))


def channels(tab, planes):
    return (1 if planes & COUNT else 0) + (2 if planes & FLOW else 0) + (tab['M'] if planes & OBJECTS else 0)


def restate_env(tab, gw, gh, planes, x, y, th, ox=None, oy=None, oth=None):
    """One env: x, y, th [N], ox, oy, oth [M] float32 (world units, radians) -> [C, gh, gw] float32."""
    out = []
    ix, iy = cells(tab, gw, gh, x, y)
    flat = iy * gw + ix
    if planes & COUNT:
        out.append(np.bincount(flat, minlength=gw * gh).astype(np.float32).reshape(1, gh, gw))
    if planes & FLOW:
        for q in quantised_headings(th):
            acc = np.zeros(gw * gh, dtype=np.int64)
            np.add.at(acc, flat, q.astype(np.int64))
            assert np.abs(acc).max(initial=0) < 2 ** 31
            plane = acc.astype(np.int32).astype(np.float32) / SCALE
            assert plane.dtype == np.float32
            out.append(plane.reshape(1, gh, gw))
    if planes & OBJECTS:
        out.append(object_masks(tab, gw, gh, ox, oy, oth)[0])
    return np.concatenate(out, 0)


def restate(tab, gw, gh, planes, x, y, th, ox=None, oy=None, oth=None):
    """x, y, th [E, N], ox, oy, oth [E, M] float32 (None without objects) -> [E, C, gh, gw] float32."""
    E = x.shape[0]
    none = [None] * E
    ox, oy, oth = (none if v is None else v for v in (ox, oy, oth))
    return np.stack([restate_env(tab, gw, gh, planes, x[e], y[e], th[e], ox[e], oy[e], oth[e]) for e in range(E)])


def plane_slices(tab, planes):
    """{plane bit: slice of its channels in the output of `planes`}."""
    at, out = 0, {}
    for bit, n in ((COUNT, 1), (FLOW, 2), (OBJECTS, tab['M'])):
        if planes & bit:
            out[bit] = slice(at, at + n)
            at += n
    return out


bits = objects_ref.bits
