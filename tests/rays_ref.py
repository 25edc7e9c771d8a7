"""Numpy restatement of kb_sense_rays' definition (include/kilobots_hip.h), shared by the range-scan tests.

Brute force: every kilobot meets every other kilobot, every fixture edge and every wall; no grid, no stencil.  With
ft = float32 every operation is its own float32 expression on float32 arrays, so each rounds on its own like the kernel's
(-ffp-contract=off), sine and cosine are the oracle library's sincosf (objects_ref.sincos) and the direction table is the
definition's (double, rounded to float32): comparisons with the device are by equality of the bit patterns.  With
ft = float64 the same formulas run on the same inputs in double, with the directions as exact as double gives them: the
quantity the float32 evaluation approximates.  The geometry comes ONLY from kb_get_outline (objects_ref.tables)."""
import math

import numpy as np

from tests.objects_ref import sincos
from tests.scenes import world  # noqa: F401

BOTS, OBJECTS, WALLS = 1, 2, 4
NONE = 1 << 40          # the code of "nothing hit" while the candidates are met: above every real code


def directions(n, ft=np.float32):
    """u_k = (cos, sin)(2 pi k / n) evaluated in double; for float32 rounded to it, the whole quarter turns exact."""
    u = np.zeros((n, 2), dtype=ft)
    for k in range(n):
        t = 2.0 * math.pi * float(k) / float(n)
        u[k] = (math.cos(t), math.sin(t))
        if (4 * k) % n == 0:
            u[k] = ((1, 0), (0, 1), (-1, 0), (0, -1))[4 * k // n]
    return u


class Scan(object):
    """The running best (t, code) of [N, K] rays."""

    def __init__(self, N, K, Rw, ft):
        self.ft, self.Rw = ft, ft(Rw)
        self.t = np.full((N, K), np.inf, dtype=ft)
        self.code = np.full((N, K), NONE, dtype=np.int64)
        self.cond = np.zeros((N, K), dtype=ft)

    def take(self, k, t, ok, cond, code):
        """Ray k of every kilobot: a candidate at t (where ok: it was not a miss) with this code (a number or [N]).  cond:
        how much an error of the candidate's (b, q) is amplified in t, kept for the winner (see disc and segment)."""
        with np.errstate(invalid='ignore'):
            hit = ok & (t <= self.Rw)
            t = np.where(t > 0, t, self.ft(0))
            better = hit & ((t < self.t[:, k]) | ((t == self.t[:, k]) & (code < self.code[:, k])))
        self.t[:, k] = np.where(better, t, self.t[:, k])
        self.code[:, k] = np.where(better, code, self.code[:, k])
        self.cond[:, k] = np.where(better, cond, self.cond[:, k])


def disc(b, q, r2):
    """(t, ok, cond) of a disc of squared radius r2 whose centre is at (b, q) along and across the ray; cond = |q| / sq, the
    slope of sq in q."""
    with np.errstate(invalid='ignore', divide='ignore'):
        h2 = r2 - q * q
        ok = h2 >= 0
        sq = np.sqrt(h2)
        t1 = b - sq
        t2 = b + sq
        ok = ok & (t2 >= 0)
        return np.where(t1 >= 0, t1, t2), ok, np.abs(q) / sq


def segment(bA, qA, bB, qB):
    """(t, ok, cond) of the segment from (bA, qA) to (bB, qB); cond = |bB - bA| / |den|, the cotangent of the angle at which
    the ray meets the segment."""
    with np.errstate(invalid='ignore', divide='ignore'):
        straddle = ((qA <= 0) & (qB >= 0)) | ((qA >= 0) & (qB <= 0))
        den = qA - qB
        sg = qA / den
        t = bA + sg * (bB - bA)
        return t, straddle & (den != 0) & (t >= 0), np.abs(bB - bA) / np.abs(den)


def restate_env(tab, x, y, th, ox, oy, oth, radius_m, bot_radius_m, n_rays, targets, ft=np.float32, with_cond=False):
    """One env: x, y, th [N], ox, oy, oth [M] float32 (world units, radians); radius_m and bot_radius_m as the host passes
    them (python floats, rounded to float32 here).  Returns (dist [N, K] of dtype ft, hit [N, K] int32), with with_cond=True also
    the winner's conditioning [N, K] (0 where nothing was hit)."""
    for v in (x, y, th, ox, oy, oth):
        assert v.dtype == np.float32
    f32 = np.float32
    N, K = x.shape[0], int(n_rays)
    S = f32(25)
    Rw = f32(radius_m) * S                  # the host constants are float32 whatever ft is: they are inputs
    rb = f32(bot_radius_m) * S
    rb2 = rb * rb
    Rc = Rw + rb
    Rc2 = Rc * Rc
    u = directions(K, ft)
    xi, yi = x.astype(ft), y.astype(ft)
    s, c = sincos(th, ft)
    s, c = s.astype(ft), c.astype(ft)
    scan = Scan(N, K, Rw, ft)

    def frame(px, py):
        """The world point(s) (px, py) ([N] or [N, J]) in every kilobot's frame: (a, l)."""
        if np.ndim(px) == 2:
            dx, dy = px - xi[:, None], py - yi[:, None]
            return c[:, None] * dx + s[:, None] * dy, c[:, None] * dy - s[:, None] * dx
        dx, dy = px - xi, py - yi
        return c * dx + s * dy, c * dy - s * dx

    def along(a, l, k):
        return a * u[k, 0] + l * u[k, 1], a * u[k, 1] - l * u[k, 0]

    if targets & BOTS and N > 1:
        ex, ey = xi[None, :] - xi[:, None], yi[None, :] - yi[:, None]
        dd = ex * ex + ey * ey
        cand = ~(dd > ft(Rc2)) & ~np.eye(N, dtype=bool)
        a, l = frame(np.broadcast_to(xi[None, :], (N, N)), np.broadcast_to(yi[None, :], (N, N)))
        for k in range(K):
            b, q = along(a, l, k)
            t, ok, cond = disc(b, q, ft(rb2))
            with np.errstate(invalid='ignore'):
                ok = ok & cand & (t <= scan.Rw)
            t = np.where(ok, np.where(t > 0, t, ft(0)), np.inf)
            j = np.argmin(t, 1)                     # (the first of equal t: the lowest index)
            rows = np.arange(N)
            scan.take(k, t[rows, j], ok[rows, j], cond[rows, j], j)
    if targets & OBJECTS:
        so_all, co_all = sincos(oth, ft)
        for fx in tab['fixtures']:
            m = fx['body']
            so, co = ft(so_all[m]), ft(co_all[m])
            code = N + 4 + m
            if fx['n'] == 0:
                r = ft(fx['radius'])
                a, l = frame(ft(ox[m]), ft(oy[m]))
                for k in range(K):
                    b, q = along(a, l, k)
                    scan.take(k, *disc(b, q, r * r), code=code)
                continue
            v = fx['verts'].astype(ft)
            wx = ft(ox[m]) + (co * v[:, 0] - so * v[:, 1])
            wy = ft(oy[m]) + (so * v[:, 0] + co * v[:, 1])
            al = [frame(wx[i], wy[i]) for i in range(fx['n'])]
            for i in range(fx['n']):
                (aA, lA), (aB, lB) = al[i], al[(i + 1) % fx['n']]
                for k in range(K):
                    bA, qA = along(aA, lA, k)
                    bB, qB = along(aB, lB, k)
                    scan.take(k, *segment(bA, qA, bB, qB), code=code)
    if targets & WALLS:
        x0, x1, y0, y1 = (ft(v) for v in tab['arena'])
        ends = [((x0, y0), (x0, y1)), ((x1, y0), (x1, y1)), ((x0, y0), (x1, y0)), ((x0, y1), (x1, y1))]
        for w, (A, B) in enumerate(ends):
            aA, lA = frame(*A)
            aB, lB = frame(*B)
            for k in range(K):
                bA, qA = along(aA, lA, k)
                bB, qB = along(aB, lB, k)
                scan.take(k, *segment(bA, qA, bB, qB), code=N + w)
    none = scan.code == NONE
    dist = np.where(none, ft(Rw), scan.t) / ft(S)
    hit = np.where(none, -1, scan.code).astype(np.int32)
    assert dist.dtype == ft
    return (dist, hit, scan.cond) if with_cond else (dist, hit)


def restate(tab, x, y, th, ox, oy, oth, radius_m, bot_radius_m, n_rays, targets, ft=np.float32):
    """x, y, th [E, N], ox, oy, oth [E, M] float32 (None without objects) -> (dist [E, N, K], hit [E, N, K])."""
    E = x.shape[0]
    none = np.zeros((E, 0), dtype=np.float32)
    ox, oy, oth = (none if v is None else v for v in (ox, oy, oth))
    envs = [restate_env(tab, x[e], y[e], th[e], ox[e], oy[e], oth[e], radius_m, bot_radius_m, n_rays, targets, ft) for e in range(E)]
    return np.stack([d for d, _ in envs]), np.stack([h for _, h in envs])


# ---- what the CPU and the GPU tests share of their scenes ----------------------------------------------------------------------
OBJECT_SCENE = dict(E=4, N=64, R=0.15, K=16)
OBJECT_SEEDS = {'disc': 31, 'boxes': 32, 'mixed': 33, 'forms': 34}


def object_scene(name):
    """(kb_config keywords, xy [E, N, 2] m, th [E, N], object xy [E, M, 2] m, object headings [E, M]) of one set of
    objects_ref.object_sets(): kilobots drawn around the objects, some inside."""
    from tests import objects_ref
    kw, centres = objects_ref.object_sets()[name]
    return (kw,) + objects_ref.spawn_over_objects(OBJECT_SCENE['E'], OBJECT_SCENE['N'], centres, OBJECT_SEEDS[name])
