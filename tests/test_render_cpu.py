"""kb_render and kb_render_default_style without a GPU: the symbols are exported, bound and declared, the defaults are the
reference's colours, the host-side validation answers in the header's order (arguments before the bound check, so none of it
needs a device), the kernel has no private segment and no spill (the code object's metadata), the Python layers validate
what they are given, and the numpy restatement (tests/render_ref.py) is the intended picture on scenes made by hand."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from tests import objects_ref
from tests import render_ref as ref
from tests.host_common import Handle, lib  # noqa: F401
from tests.sensing_common import f32, kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_BOT = 0.0165


def test_symbols_are_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, 'include', 'kilobots_hip.h')).read()
    m = re.search(r'\bint\s+kb_render\s*\(([^)]*)\)\s*;', hdr)
    assert m and len(m.group(1).split(',')) == 9
    assert re.search(r'\bint\s+kb_render_default_style\s*\(\s*kb_render_style\s*\*\s*out\s*\)\s*;', hdr)
    assert re.search(r'\}\s*kb_render_style\s*;', hdr)
    for name, nargs in (('kb_render', 9), ('kb_render_default_style', 1)):
        assert name in nat.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == nargs
    assert set(re.findall(r'\b(kb_[a-z_]+)\s*\(', hdr)) == set(nat.EXPORTS)
    for name, value in (('OBJECTS', 1), ('BOTS', 2), ('LIGHT', 4), ('MAX_SIDE', 2048)):
        assert re.search(r'#define\s+KB_RENDER_%s\s+%d\b' % (name, value), hdr) and getattr(nat, 'RENDER_' + name) == value
    assert (ref.OBJECTS, ref.BOTS, ref.LIGHT) == (nat.RENDER_OBJECTS, nat.RENDER_BOTS, nat.RENDER_LIGHT)
    # the ctypes image of kb_render_style: five colours, alpha, eight object colours, all bytes
    assert C.sizeof(nat.KbRenderStyle) == 5 * 3 + 1 + 3 * nat.MAX_OBJECTS
    assert [n for n, _ in nat.KbRenderStyle._fields_] == ['table', 'body', 'ring', 'mark', 'light', 'light_alpha', 'obj']


def test_default_style(lib):
    st = nat.KbRenderStyle()
    C.memset(C.byref(st), 0xEE, C.sizeof(st))
    assert lib.kb_render_default_style(C.byref(st)) == nat.KB_OK
    assert list(st.table) == [255, 255, 255] and list(st.body) == [150, 150, 150] and list(st.ring) == [100, 100, 100]
    assert list(st.mark) == [255, 255, 255] and list(st.light) == [255, 255, 30] and st.light_alpha == 150
    assert [list(st.obj[m]) for m in range(nat.MAX_OBJECTS)] == [[93, 133, 195]] * nat.MAX_OBJECTS
    lib.kb_sense_neighbors(None, 0.07, 8, None, None, None, None)      # (leaves a message that the next call must replace)
    assert lib.kb_render_default_style(None) == nat.KB_EINVAL and b'kb_render_default_style' in lib.kb_last_error()
    # the restatement's defaults are these, and render_style() overlays a dict on them
    d = ref.DEFAULT_STYLE
    assert [list(getattr(st, k)) for k in ('table', 'body', 'ring', 'mark', 'light')] == [list(d[k]) for k in ('table', 'body', 'ring', 'mark', 'light')]
    assert st.light_alpha == d['light_alpha'] and [list(st.obj[m]) for m in range(8)] == [list(c) for c in d['obj']]
    own = nat.render_style({'ring': (1, 2, 3), 'light_alpha': 7, 'obj': [(9, 8, 7), (6, 5, 4)]})
    assert list(own.ring) == [1, 2, 3] and own.light_alpha == 7 and list(own.obj[1]) == [6, 5, 4] and list(own.obj[2]) == [93, 133, 195]
    assert list(own.table) == [255, 255, 255]
    for bad in ({'rim': (1, 2, 3)}, {'ring': (1, 2)}, {'ring': (1, 2, 256)}, {'light_alpha': 256}, {'obj': [(1, 2, 3)] * 9}):
        with pytest.raises(ValueError):
            nat.render_style(bad)


def test_argument_errors_come_in_the_stated_order(lib):
    """Nothing here launches: the pointers are never dereferenced on the host.  NULL sim / d_rgb, then the layers, then the
    size, and only then the unbound handle."""
    out = C.c_void_p(0x1001)        # (d_rgb is byte aligned)
    with Handle(lib) as h:
        bad = [
            ('NULL sim', (None, 8, 8, 7, None, None, None, out), b'NULL'),
            ('NULL d_rgb', (h, 8, 8, 7, None, None, None, None), b'NULL'),
            ('NULL d_rgb before bad layers', (h, 8, 8, 0, None, None, None, None), b'NULL'),
            ('NULL sim before a bad size', (None, 0, 8, 7, None, None, None, out), b'NULL'),
            ('no layer', (h, 8, 8, 0, None, None, None, out), b'layers'),
            ('an unknown layer', (h, 8, 8, 8, None, None, None, out), b'layers'),
            ('negative layers', (h, 8, 8, -1, None, None, None, out), b'layers'),
            ('layers before the size', (h, 0, 8, 16, None, None, None, out), b'layers'),
            ('width = 0', (h, 0, 8, 7, None, None, None, out), b'KB_RENDER_MAX_SIDE'),
            ('height = 0', (h, 8, 0, 2, None, None, None, out), b'KB_RENDER_MAX_SIDE'),
            ('width too large', (h, 2049, 8, 1, None, None, None, out), b'KB_RENDER_MAX_SIDE'),
            ('height too large', (h, 8, 2049, 4, None, None, None, out), b'KB_RENDER_MAX_SIDE'),
        ]
        for what, args, word in bad:
            lib.kb_sense_neighbors(None, 0.07, 8, out, out, out, None)     # (leaves a message that the next call must replace)
            assert lib.kb_render(*args, None) == nat.KB_EINVAL, what
            msg = lib.kb_last_error()
            assert msg and b'kb_render' in msg and word in msg, (what, msg)
        # legal arguments reach the bound check: every layer mask, the largest and the smallest frame, a style and colour arrays
        st = nat.render_style()
        for args in ((8, 8, 7, None, None, None), (2048, 2048, 1, None, None, None), (1, 1, 2, C.byref(st), out, out), (1200, 900, 4, None, out, None),
                     (64, 48, 3, None, None, out), (64, 48, 5, None, None, None), (64, 48, 6, None, None, None)):
            assert lib.kb_render(h, *args, out, None) == nat.KB_ENOTBOUND, args
            assert b'kb_render' in lib.kb_last_error() and b'kb_bind' in lib.kb_last_error()


def test_check_render_and_the_env_layers():
    import torch
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    from tests.oracle_backend import OracleBackend
    assert nat.check_render(64, 48, ('objects', 'bots', 'light')) == (64, 48, 7)
    assert nat.check_render(1, 2048, ['light', 'objects']) == (1, 2048, 5) and nat.check_render(2048, 1, 'bots') == (2048, 1, 2)
    assert nat.check_render(3, 2, nat.RENDER_BOTS | nat.RENDER_LIGHT) == (3, 2, 6)
    for bad in ((0, 4, 2), (4, 0, 2), (2049, 4, 2), (4, 2049, 2), (4, 4, 0), (4, 4, 8), (4, 4, -1), (4, 4, ()), (4, 4, ('heat',)), (4, 4, 'bot'),
                (4, 4, True)):
        with pytest.raises(ValueError):
            nat.check_render(*bad)
    env = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3)
    assert env.render_size is None
    with pytest.raises(ValueError):
        env.render()
    with pytest.raises(ValueError):
        env.render('rgb_array')
    with pytest.raises(NotImplementedError):
        env.render('human')
    for bad in (5, (64,), (64, 48, 3), (0, 48), (64, 2049), ('a', 'b')):
        with pytest.raises(ValueError):
            BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, render_size=bad)
    ok = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3, render_size=[64, 48])
    assert ok.render_size == (64, 48)
    with pytest.raises(NotImplementedError):
        ok.render('human')
    a = torch.zeros(3, 16, 2)
    a[..., 0] = 0.01
    assert torch.equal(ok.reset(), env.reset())
    so, se = ok.step(a), env.step(a)
    assert torch.equal(so[0], se[0]) and so[3] == {} and se[3] == {}


def test_kilobots_env_render_modes_without_a_gpu():
    from tests.oracle_backend import OracleBackend
    from tests.env_scenes import VelEnv
    assert VelEnv.metadata['render.modes'] == ['human', 'rgb_array']
    env = VelEnv(sim_factory=OracleBackend)
    assert env.render_mode == 'human'
    env.reset()
    for mode in (None, 'human', 'rgb_array', 'ansi'):       # (the oracle backend has no render)
        with pytest.raises(NotImplementedError):
            env.render(mode)


def test_kernel_uses_no_scratch_and_spills_nothing(lib):
    found = kernel_metadata('kb_render')
    assert len(found) == 1 and 'kb_render_kernel' in found[0][0], found
    for name, fields in found:
        for key in ('.private_segment_fixed_size', '.sgpr_spill_count', '.vgpr_spill_count'):
            assert fields[key] == 0, (name, key, fields[key])


def test_band_rule():
    """The host rule as _native.render_bands restates it: one band for the frames of a policy, several with a partial last
    band for the frame the GPU tests use for that, every band within 8192 pixels and every row in exactly one band."""
    assert nat.render_bands(1024, 2.0, 1.5, R_BOT, 64, 48) == (1, 48)
    assert nat.render_bands(1024, 2.0, 1.5, R_BOT, 128, 96) == (2, 48)
    assert nat.render_bands(16, 2.0, 1.5, R_BOT, 1, 1) == (1, 1)
    assert nat.render_bands(64, 2.0, 1.5, R_BOT, 400, 300) == (15, 20)          # (no partial band: the GPU tests take 297 rows)
    bands, rows = nat.render_bands(64, 2.0, 1.5, R_BOT, 400, 297)
    assert bands >= 2 and (bands - 1) * rows < 297 < bands * rows
    for n in (1, 64, 1024):
        for w, h in ((1, 1), (3, 2), (127, 95), (400, 300), (1200, 900), (2048, 2048), (1, 2048), (2048, 1)):
            bands, rows = nat.render_bands(n, 2.0, 1.5, R_BOT, w, h)
            assert rows >= 1 and (rows * w <= 8192 or rows == 1) and (bands - 1) * rows < h <= bands * rows


# ---- the restatement is the intended picture ------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small_tab(lib):
    """An arena of 0.1 m x 0.076 m: at 50 x 38 a pixel is 2 mm, a kilobot (r + 2 mm = 18.5 mm) 18 pixels across."""
    with Handle(lib, world_width=0.1, world_height=0.076) as h:
        return objects_ref.tables(nat.outline(h))


def classify(px, py, x, y, th):
    """The definition for one kilobot and one pixel in plain Python floats: None outside, else 'mark' | 'ring' | 'body'."""
    ro = R_BOT + 0.002
    Ro, Ri, Lf, Hw = ro * 25.0, (ro - 0.005) * 25.0, (R_BOT - 0.005) * 25.0, 0.0025 * 25.0
    qx, qy = px - x, py - y
    dd = qx * qx + qy * qy
    if not dd <= Ro * Ro:
        return None
    a, l = math.cos(th) * qx + math.sin(th) * qy, math.cos(th) * qy - math.sin(th) * qx
    if 0 <= a <= Lf and abs(l) <= Hw:
        return 'mark'
    return 'ring' if dd > Ri * Ri else 'body'


def test_one_kilobot_at_the_origin(small_tab):
    W, H = 50, 38
    style = dict(table=(0, 0, 0), body=(10, 0, 0), ring=(0, 20, 0), mark=(0, 0, 30))
    img = ref.restate_env(small_tab, W, H, ref.BOTS, R_BOT, f32([0.0]), f32([0.0]), f32([0.0]), style=style)
    assert img.dtype == np.uint8 and img.shape == (H, W, 3)
    xmin, xmax, ymin, ymax = (float(v) for v in small_tab['arena'])
    cw, ch = (xmax - xmin) / W, (ymax - ymin) / H
    i, k = 25, 19           # the pixel whose half-open cell [0, cw) x [0, ch) holds the centre: its own centre is 1 mm ahead, 1 mm to the left
    px, py = ref.centres(small_tab, R_BOT, W, H)
    assert abs(px[i] - 0.025) < 1e-6 and abs(py[H - 1 - k] - 0.025) < 1e-6
    assert img[H - 1 - k, i].tolist() == [0, 0, 30] and img[H - 1 - k, i - 1].tolist() == [10, 0, 0]      # (behind the centre: body)
    assert np.array_equal(img, img[::-1])                               # theta = 0: y -> -y maps the picture onto itself
    want = {None: 0, 'body': 0, 'ring': 0, 'mark': 0}
    for j in range(H):
        for c in range(W):
            want[classify(xmin + (c + 0.5) * cw, ymin + (H - 1 - j + 0.5) * ch, 0.0, 0.0, 0.0)] += 1
    got = {name: int((img == np.array(col, dtype=np.uint8)).all(-1).sum()) for name, col in (('body', (10, 0, 0)), ('ring', (0, 20, 0)), ('mark', (0, 0, 30)))}
    print('pixels', got)
    assert got == {k_: v for k_, v in want.items() if k_} and want[None] + sum(got.values()) == W * H
    # 18.5 mm of radius at 2 mm per pixel: about pi 9.25^2 = 269 pixels, of which the 5 mm ring is 1 - (13.5 / 18.5)^2 = 47 %
    assert 250 <= sum(got.values()) <= 290 and 0.40 <= got['ring'] / sum(got.values()) <= 0.54 and 8 <= got['mark'] <= 24
    # a quarter turn: the mark now runs up the picture
    up = ref.restate_env(small_tab, W, H, ref.BOTS, R_BOT, f32([0.0]), f32([0.0]), f32([math.pi / 2]), style=style)
    assert up[H - 1 - k, i].tolist() == [0, 0, 30] and up[H - 1 - k - 3, i].tolist() == [0, 0, 30] and img[H - 1 - k - 3, i].tolist() == [10, 0, 0]


def test_two_overlapping_kilobots(small_tab):
    W, H = 50, 38
    x, y, th = f32([-0.2, 0.2]), f32([0.05, -0.05]), f32([0.3, 2.0])
    body, mark = np.array([0x110000, 0x000022]), np.array([0x330000, 0x000044])
    both = ref.restate_env(small_tab, W, H, ref.BOTS, R_BOT, x, y, th, body=body, mark=mark)
    only = [ref.restate_env(small_tab, W, H, ref.BOTS, R_BOT, x[b:b + 1], y[b:b + 1], th[b:b + 1], body=body[b:b + 1], mark=mark[b:b + 1]) for b in (0, 1)]
    table = np.array([255, 255, 255], dtype=np.uint8)
    cov = [~(o == table).all(-1) for o in only]
    overlap = cov[0] & cov[1]
    assert overlap.sum() > 50 and (cov[0] & ~cov[1]).sum() > 20
    assert np.array_equal(both[cov[1]], only[1][cov[1]])                    # wherever the higher index covers, it is drawn
    assert np.array_equal(both[cov[0] & ~cov[1]], only[0][cov[0] & ~cov[1]])
    assert (both[~cov[0] & ~cov[1]] == table).all()
    assert (only[0][overlap] != only[1][overlap]).any(-1).sum() > 20        # (the two pictures do differ on the overlap)


def test_light_blend_by_hand(lib):
    with Handle(lib) as h:
        tab = objects_ref.tables(nat.outline(h))
    lights = ([0.2], f32([0.5]), f32([-0.25]))
    img = ref.restate_env(tab, 64, 48, ref.ALL, R_BOT, f32([20.0]), f32([15.0]), f32([0.0]), lights=lights, style=dict(table=(100, 100, 100)))
    px, py = ref.centres(tab, R_BOT, 64, 48)
    i, j = int(np.argmin(np.abs(px - 12.5))), int(np.argmin(np.abs(py + 6.25)))
    # (255 * 150 + 100 * 105 + 127) // 255 = 48877 // 255 = 191;  (30 * 150 + 100 * 105 + 127) // 255 = 15127 // 255 = 59
    assert img[j, i].tolist() == [191, 191, 59]
    assert img[0, 0].tolist() == [100, 100, 100]
    inside = (img == np.array([191, 191, 59], dtype=np.uint8)).all(-1).sum()
    assert abs(inside - math.pi * 5.0 ** 2 / ((50.0 / 64) * (37.5 / 48))) < 12      # a disc of 5 world units in pixels
    off = ref.restate_env(tab, 64, 48, ref.OBJECTS | ref.BOTS, R_BOT, f32([20.0]), f32([15.0]), f32([0.0]), lights=lights, style=dict(table=(100, 100, 100)))
    assert (off[j, i] == 100).all()
    # a second component over the first blends the blended colour again
    two = ref.restate_env(tab, 64, 48, ref.LIGHT, R_BOT, f32([20.0]), f32([15.0]), f32([0.0]), lights=([0.2, 0.1], f32([0.5, 0.5]), f32([-0.25, -0.25])),
                          style=dict(table=(100, 100, 100)))
    assert two[j, i].tolist() == [(255 * 150 + 191 * 105 + 127) // 255, (255 * 150 + 191 * 105 + 127) // 255, (30 * 150 + 59 * 105 + 127) // 255]


def test_a_higher_object_paints_over_a_lower_one(lib):
    kw = dict(num_objects=2, obj_shape=[1, 0], obj_verts=[objects_ref.box(0.3, 0.2)], obj_radius=[0.0, 0.05])
    with Handle(lib, **kw) as h:
        tab = objects_ref.tables(nat.outline(h))
    style = dict(obj=[(200, 0, 0), (0, 0, 200)])
    ox, oy, oth = f32([0.0, 1.0]), f32([0.0, 0.5]), f32([0.2, 0.0])
    img = ref.restate_env(tab, 128, 96, ref.OBJECTS, R_BOT, f32([0.0]), f32([0.0]), f32([0.0]), ox, oy, oth, style=style)
    px, py = ref.centres(tab, R_BOT, 128, 96)
    at = lambda x, y: img[int(np.argmin(np.abs(py - y))), int(np.argmin(np.abs(px - x)))].tolist()
    assert at(1.0, 0.5) == [0, 0, 200]          # the disc (object 1) lies inside the box (object 0) and is drawn over it
    assert at(-2.5, -1.0) == [200, 0, 0] and at(10.0, 10.0) == [255, 255, 255]
    assert at(0.0, 0.0) == [0, 0, 200] or at(0.0, 0.0) == [200, 0, 0]
    swapped = ref.restate_env(tab, 128, 96, ref.OBJECTS | ref.BOTS, R_BOT, f32([1.0]), f32([0.5]), f32([0.0]), ox, oy, oth, style=style)
    assert swapped[int(np.argmin(np.abs(py - 0.5))), int(np.argmin(np.abs(px - 1.0)))].tolist() != [0, 0, 200]      # a kilobot replaces the object colour
