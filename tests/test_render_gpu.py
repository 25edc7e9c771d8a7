"""kb_render on the GPU against the numpy restatement of its definition (tests/render_ref.py), whose arena and fixtures come
from kb_get_outline alone, whose sine and cosine are the oracle library's and whose object layer is the inside flag of
tests/objects_ref.py.

Everything is compared for equality of the bytes: every operation of the definition is one fp32 operation rounded on its
own, the blend is integer arithmetic, on the device and in the restatement.  No tolerances."""
import numpy as np
import pytest
import torch

from gym_kilobots_amd import _native as nat
from tests import objects_ref
from tests import render_ref as ref
from tests import scenes
from tests.gpu_common import cpu, dev
from tests.sensing_checks import check_render as check, colour_words as words, want_render as want
from tests.sensing_common import f32, make_sim

pytestmark = pytest.mark.gpu

NAN, INF = float('nan'), float('inf')
SETS = objects_ref.object_sets()
# one pixel; ragged byte stores; rows that are a multiple of 16 bytes; a row stride of 381 bytes, no alignment anywhere
SIZES = [(1, 1), (3, 2), (7, 5), (64, 48), (128, 96), (127, 95)]
BANDED = (400, 297)     # at N = 64: 15 bands of 20 rows, the last of 17 (400 x 300 would be 15 full bands)
OWN_STYLE = dict(table=(12, 34, 56), body=(1, 2, 3), ring=(200, 100, 0), mark=(9, 250, 9), light=(0, 128, 255), light_alpha=77,
                 obj=[(10 * m + 5, 255 - 20 * m, 7 * m) for m in range(8)])


def colours(E, N, seed):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 1 << 24, size=(E, N)), rng.randint(0, 1 << 24, size=(E, N)) | 0x7F000000       # (the top byte is ignored)


def lit(E, seed, **kw):
    """Keywords of a circular light, and its positions [E, 2] in metres."""
    rng = np.random.RandomState(seed)
    return dict(light_type=nat.LIGHT_CIRCULAR, light_radius=0.2, **kw), rng.uniform(-0.6, 0.6, size=(E, 2))


def place_light(g, xy):
    g.light_x.copy_(dev(f32(xy[..., 0]).reshape(tuple(g.light_x.shape))))
    g.light_y.copy_(dev(f32(xy[..., 1]).reshape(tuple(g.light_y.shape))))


def make_scene(E, N, scene, seed):
    """The scenes of test_grid_gpu.py, every one under a circular light."""
    lkw, lxy = lit(E, seed + 100)
    if scene == 'gaussian':
        xy, th = scenes.gaussian_spawn(E, N, sigma=0.2, seed=seed)
        th = np.random.RandomState(seed).uniform(-np.pi, np.pi, size=(E, N))
        g = make_sim(E, N, xy, th, **lkw)
    else:
        kw, centres = SETS[scene]
        xy, th, objs, oth = objects_ref.spawn_over_objects(E, N, centres, seed)
        g = make_sim(E, N, xy, th, **kw, **lkw)
        g.set_objects_m(objs, oth)
    place_light(g, lxy)
    return g


CASES = [(E, N, scene) for E, N in [(5, 1), (2, 7), (8, 64), (3, 333), (2, 1024)] for scene in ['gaussian', 'disc', 'boxes', 'mixed', 'forms']]


@pytest.mark.parametrize('E,N,scene', CASES)
def test_frames_equal_the_restatement(E, N, scene):
    """Every size of SIZES on one sim per case, all three layers; per-kilobot colour arrays on every other case.  On one case
    also each layer alone and a style of its own.  From 64 x 48 upward the objects, the kilobots and the light all show."""
    at = CASES.index((E, N, scene))
    g = make_scene(E, N, scene, seed=E * N + 1)
    body, mark = colours(E, N, at) if at % 2 else (None, None)
    for width, height in SIZES:
        w = check(g, width, height, body=body, mark=mark, what=scene)
        if width >= 64:
            flat = w.reshape(E, -1, 3)
            assert ((flat != 255).any(-1).sum(1) > 0).all()                # something is drawn in every env
            assert (flat == 255).all(-1).any()                              # and some table is left
    if (E, N, scene) == (8, 64, 'mixed'):
        for layers in (ref.OBJECTS, ref.BOTS, ref.LIGHT, ref.OBJECTS | ref.LIGHT):
            alone = check(g, 127, 95, layers, body=body, mark=mark, what='layers')
            assert (alone != 255).any()
        own = check(g, 128, 96, style=OWN_STYLE, what='style')
        # the table, the ring, the body, the mark and all eight objects are in the picture in their own colours
        for col in [OWN_STYLE[k] for k in ('table', 'ring', 'body')] + OWN_STYLE['obj']:
            assert (own == np.array(col, dtype=np.uint8)).all(-1).any(), col


def test_lights():
    E, N = 3, 64
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.25, seed=31)
    # a circular light
    lkw, lxy = lit(E, 5)
    g = make_sim(E, N, xy, th, **lkw)
    place_light(g, lxy)
    for width, height in ((64, 48), (127, 95)):
        w = check(g, width, height, what='circular')
        assert (w != check(g, width, height, ref.OBJECTS | ref.BOTS, what='circular, off')).any()
    # a composite of a circular and a momentum light whose discs overlap: the second blends over the first
    comp = make_sim(E, N, xy, th, light_type=nat.LIGHT_COMPOSITE, light_count=2, light_kind=[nat.LIGHT_CIRCULAR, nat.LIGHT_MOMENTUM],
                    lightc_radius=[0.2, 0.15])
    place_light(comp, np.stack([lxy, lxy + np.array([0.1, 0.05])], 1))
    w = check(comp, 128, 96, what='composite')
    once = (255 * 150 + 255 * 105 + 127) // 255, (30 * 150 + 255 * 105 + 127) // 255
    twice = (30 * 150 + once[1] * 105 + 127) // 255
    assert (w == np.array([255, 255, once[1]], dtype=np.uint8)).all(-1).any() and (w == np.array([255, 255, twice], dtype=np.uint8)).all(-1).any()
    check(comp, 7, 5, what='composite')
    # a gradient light and no light: the layer draws nothing, the frame is the one without the bit
    grad = make_sim(E, N, xy, th, light_type=nat.LIGHT_GRADIENT)
    none = make_sim(E, N, xy, th)
    for h in (grad, none):
        w = check(h, 64, 48, what='no positional light')
        assert np.array_equal(w, check(h, 64, 48, ref.OBJECTS | ref.BOTS, what='no positional light, off'))
        assert (cpu(h.render(64, 48, 'light')) == 255).all()


def search_x(px, py, y, R2, x_true, x_false):
    """The float32 x nearest to x_false for which a kilobot at (x, y) still has dd <= R2 at the pixel (px, py), and its
    neighbour towards x_false, for which it no longer has: bisection over the floats between x_true and x_false."""
    def inside(x):
        qx, qy = px - x, py - y
        return bool(qx * qx + qy * qy <= R2)
    a, b = f32(x_true), f32(x_false)
    assert inside(a) and not inside(b)
    while np.nextafter(a, b) != b:
        mid = f32((np.float64(a) + np.float64(b)) / 2)
        if mid == a or mid == b:
            break
        if inside(mid):
            a = mid
        else:
            b = mid
    assert np.nextafter(a, b) == b and inside(a) and not inside(b)
    return a, b


def test_constructed_cases():
    """One env of 64 at 256 x 192 (a kilobot is about 17 pixels); the first kilobots sit on the special points, the rest in a
    corner of their own.  Every case is asserted on the restatement before the device is compared with it."""
    N, W, H = 64, 256, 192
    g = make_sim(1, N)
    tab = objects_ref.tables(g.outline())
    r = g.cfg.bot_radius
    c = ref.constants(tab, r, W, H)
    px, py = ref.centres(tab, r, W, H)
    rng = np.random.RandomState(11)
    x, y, th = rng.uniform(-22.0, -12.0, N), rng.uniform(-16.0, -8.0, N), rng.uniform(-np.pi, np.pi, N)
    body, mark = colours(1, N, 3)
    body, mark = body[0] & 0xFFFFFF, mark[0] & 0xFFFFFF
    rgb = lambda wd: [(int(wd) >> 16) & 255, (int(wd) >> 8) & 255, int(wd) & 255]
    # 0: centred on a pixel centre, heading along x: that pixel has a = l = 0 and is the mark
    x[0], y[0], th[0] = px[200], py[20], 0.0
    # 1..10: a pile of ten coincident kilobots on a pixel centre, the top one heading along x
    jp, ip = 40, 150
    x[1:11], y[1:11], th[10] = px[ip], py[jp], 0.0
    # 11..14: half outside each wall; 15 far outside; 16 a NaN x; 17 an infinite y
    x[11:15], y[11:15] = [-25.0, 25.0, 3.0, -3.0], [2.0, -2.0, -18.75, 18.75]
    x[15], y[15] = 400.0, -300.0
    x[16], y[16] = NAN, 1.0
    x[17], y[17] = 0.0, INF
    # 18: a NaN heading
    x[18], y[18], th[18] = 15.0, -10.0, NAN
    # 19..22: pixels on either side of dd == Ro2 and of dd == Ri2 by one ulp of the kilobot's x; the kilobot is to the right of
    # the pixel and heads along x, so that the pixel is behind it: no mark
    spots = [(30, 100, c['Ro2'], +1), (60, 100, c['Ro2'], +1), (90, 100, c['Ri2'], +1), (120, 100, c['Ri2'], +1)]
    pairs = []
    for k, (j, i, R2, _) in enumerate(spots):
        yy = f32(py[j] + f32(0.05))
        a, b = search_x(px[i], py[j], yy, R2, px[i] + f32(0.2), px[i] + f32(0.6))
        pairs.append((a, b))
        x[19 + k], y[19 + k], th[19 + k] = (a if k % 2 == 0 else b), yy, 0.0
    X, Y, T = f32(x[None]), f32(y[None]), f32(th[None])
    g.x.copy_(dev(X)); g.y.copy_(dev(Y)); g.theta.copy_(dev(T))
    w = ref.restate(tab, W, H, ref.ALL, r, X, Y, T, body=body[None], mark=mark[None])[0]
    assert w[20, 200].tolist() == rgb(mark[0])
    pile = w[jp - 3:jp + 4, ip - 3:ip + 4].reshape(-1, 3).tolist()
    assert all(p in (rgb(body[10]), rgb(mark[10]), [100, 100, 100], [255, 255, 255]) for p in pile) and rgb(body[10]) in pile and rgb(mark[10]) in pile
    for b in range(1, 10):
        assert not (w == np.array(rgb(body[b]), dtype=np.uint8)).all(-1).any() and not (w == np.array(rgb(mark[b]), dtype=np.uint8)).all(-1).any()
    # the halves inside the walls are drawn up to the edge pixels
    assert w[int(np.argmin(np.abs(py - 2.0))), 0].tolist() != [255, 255, 255] and w[int(np.argmin(np.abs(py + 2.0))), W - 1].tolist() != [255, 255, 255]
    assert w[H - 1, int(np.argmin(np.abs(px - 3.0)))].tolist() != [255, 255, 255] and w[0, int(np.argmin(np.abs(px + 3.0)))].tolist() != [255, 255, 255]
    # the three that are nowhere paint nothing: without them the frame is the same
    keep = np.array([b for b in range(N) if b not in (15, 16, 17)])
    assert np.array_equal(w, ref.restate(tab, W, H, ref.ALL, r, X[:, keep], Y[:, keep], T[:, keep], body=body[None, keep], mark=mark[None, keep])[0])
    # the NaN heading: its body and the ring, never its mark
    assert (w == np.array(rgb(body[18]), dtype=np.uint8)).all(-1).sum() > 3 and not (w == np.array(rgb(mark[18]), dtype=np.uint8)).all(-1).any()
    # the one-ulp pairs
    (j0, i0, _, _), (j1, i1, _, _), (j2, i2, _, _), (j3, i3, _, _) = spots
    assert w[j0, i0].tolist() == [100, 100, 100] and w[j1, i1].tolist() == [255, 255, 255]      # just inside Ro2: the ring; just outside: the table
    assert w[j2, i2].tolist() == rgb(body[21]) and w[j3, i3].tolist() == [100, 100, 100]        # just inside Ri2: the body; just outside: the ring
    check(g, W, H, body=body[None], mark=mark[None], what='constructed', w=w[None])
    for size in ((127, 95), (64, 48)):
        check(g, *size, body=body[None], mark=mark[None], what='constructed')


def test_long_cell_chains():
    """All 1024 kilobots of one env within 4 mm of one point, next to a spread-out env: every pixel near the point walks a
    chain of 1024, and the highest index that covers it wins."""
    E, N = 2, 1024
    xy, th = scenes.gaussian_spawn(E, N, sigma=0.3, seed=77)
    rng = np.random.RandomState(2)
    xy[0] = np.array([0.1333, -0.0871]) + rng.uniform(-0.004, 0.004, size=(N, 2))
    th = rng.uniform(-np.pi, np.pi, size=(E, N))
    g = make_sim(E, N, xy, th)
    body, mark = colours(E, N, 9)
    for width, height in ((128, 96), (127, 95)):
        w = check(g, width, height, body=body, mark=mark, what='one point')
        assert (w[0] != 255).any(-1).sum() < 40 < (w[1] != 255).any(-1).sum()


def test_every_byte_is_written():
    """out= full of 0xAB comes back as the restatement, on a 16-byte aligned buffer and on one that starts a byte behind such
    a boundary, twice, and from a side stream; a bad out raises."""
    E, N = 3, 333
    g = make_scene(E, N, 'boxes', seed=4)
    body, mark = colours(E, N, 1)
    wb, wm = words(body), words(mark)
    for width, height in ((64, 48), (7, 5), (127, 95), (1, 1)):
        w = want(g, width, height, body=body, mark=mark)
        n = E * height * width * 3
        for off in (0, 1):
            buf = torch.full((n + off,), 0xAB, dtype=torch.uint8, device='cuda')
            out = buf[off:].view(E, height, width, 3)
            assert out.data_ptr() % 16 == off
            for _ in range(2):      # reused: the same answer twice
                got = g.render(width, height, body_rgb=wb, mark_rgb=wm, out=out)
                assert got.data_ptr() == out.data_ptr()
                assert np.array_equal(cpu(out), w)
                out.fill_(0xAB)
            g.render(width, height, body_rgb=wb, mark_rgb=wm, out=out)
            assert np.array_equal(cpu(out), w) and (off == 0 or int(buf[0]) == 0xAB)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        s = g.render(127, 95, body_rgb=wb, mark_rgb=wm)
    side.synchronize()
    assert np.array_equal(cpu(s), want(g, 127, 95, body=body, mark=mark))
    for bad in (torch.zeros(E, 48, 64, 3, dtype=torch.uint8), torch.zeros(E, 64, 48, 3, dtype=torch.uint8, device='cuda'),
                torch.zeros(E, 48, 64, 3, device='cuda'), torch.zeros(E, 48, 64, 4, dtype=torch.uint8, device='cuda')[..., :3],
                torch.zeros(E - 1, 48, 64, 3, dtype=torch.uint8, device='cuda')):
        with pytest.raises(ValueError):
            g.render(64, 48, out=bad)
    for bad in (torch.zeros(E, N, device='cuda'), torch.zeros(E, N + 1, dtype=torch.int32, device='cuda'), torch.zeros(E, N, dtype=torch.int32)):
        with pytest.raises(ValueError):
            g.render(64, 48, body_rgb=bad)
    with pytest.raises(ValueError):
        g.render(64, 48, style={'rim': (1, 2, 3)})


def test_after_motion_and_untouched_state():
    """64 velocity kilobots push four boxes for 20 steps of 10 substeps; the frame taken before no longer holds, the one
    taken after is the restatement on the state the step left, and rendering changes no state tensor."""
    E, N = 2, 64
    kw, centres = SETS['boxes']
    xy, _ = scenes.gaussian_spawn(E, N, sigma=0.3, seed=63)
    g = make_sim(E, N, xy, scenes.toward_objects_theta(xy), **kw)
    g.set_objects_m(np.tile(centres[None], (E, 1, 1)), np.tile(np.array([0.4, 0.0, -1.2, 0.8])[None], (E, 1)))
    before = check(g, 128, 96, what='before motion')
    a = torch.zeros(E, N, 2, device='cuda')
    a[..., 0] = 0.01
    for _ in range(20):
        g.step(10, actions=a)
    fields = ('x', 'y', 'theta', 'ox', 'oy', 'otheta', 'ovx', 'ovy', 'ow', 'v', 'w', 'status', 'ws_cnt', 'ows_acc')
    torch.cuda.synchronize()
    kept = {f: getattr(g, f).clone() for f in fields}
    after = check(g, 128, 96, what='after motion')
    assert (before != after).any()
    torch.cuda.synchronize()
    for f in fields:
        assert torch.equal(kept[f].view(torch.uint8), getattr(g, f).view(torch.uint8)), f


def test_several_bands_with_a_partial_last_band():
    width, height = BANDED
    N = 64
    kw, centres = SETS['mixed']
    lkw, lxy = lit(1, 8)
    xy, th, objs, oth = objects_ref.spawn_over_objects(1, N, centres, 21, sigma=0.2)
    g = make_sim(1, N, xy, th, **kw, **lkw)
    g.set_objects_m(objs, oth)
    place_light(g, lxy)
    bands, rows = nat.render_bands(N, g.cfg.world_width, g.cfg.world_height, g.cfg.bot_radius, width, height)
    assert bands >= 2 and (bands - 1) * rows < height < bands * rows
    body, mark = colours(1, N, 5)
    check(g, width, height, body=body, mark=mark, what='bands')
    buf = torch.full((height * width * 3 + 1,), 0xAB, dtype=torch.uint8, device='cuda')      # (no band starts on 16 bytes)
    out = buf[1:].view(1, height, width, 3)
    g.render(width, height, out=out)
    assert np.array_equal(cpu(out), want(g, width, height))


def test_the_reference_screen():
    """1200 x 900, the reference's screen: one env of 16 kilobots and one box."""
    N = 16
    xy, th = scenes.gaussian_spawn(1, N, sigma=0.2, seed=6)
    th = np.random.RandomState(6).uniform(-np.pi, np.pi, size=(1, N))
    g = make_sim(1, N, xy, th, num_objects=1, obj_shape=[1], obj_verts=[objects_ref.box(0.15, 0.1)])
    g.set_objects_m(np.array([[[0.3, 0.2]]]), np.array([[0.5]]))
    w = check(g, 1200, 900, what='screen')
    assert (w == np.array([93, 133, 195], dtype=np.uint8)).all(-1).sum() > 0.8 * 0.15 * 0.1 * 600 * 600
    assert (w == 150).all(-1).sum() > 8 * 300      # bodies of several kilobots, about pi 8.1^2 pixels each


def test_batched_env_render():
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    E, N = 4, 64
    kw, centres = SETS['boxes']
    objs = np.tile(centres[None], (E, 1, 1))
    env = BatchedKilobotsEnv(E, N, seed=3, spawn_std=0.12, render_size=(64, 48), **kw)
    plain = BatchedKilobotsEnv(E, N, seed=3, spawn_std=0.12, **kw)
    for e in (env, plain):
        e.sim.set_objects_m(objs)
    assert torch.equal(env.reset(), plain.reset())
    a = dev(scenes.random_actions(E, N, seed=20))
    obs, rew, done, info = env.step(a)
    pobs, prew, pdone, pinfo = plain.step(a)
    assert info == {} and pinfo == {} and torch.equal(obs, pobs) and torch.equal(rew, prew) and torch.equal(done, pdone)
    frame = env.render('rgb_array')
    assert frame.dtype == torch.uint8 and tuple(frame.shape) == (E, 48, 64, 3) and frame.is_cuda
    assert torch.equal(frame, env.sim.render(64, 48)) and torch.equal(frame, env.render())
    assert np.array_equal(cpu(frame), want(env.sim, 64, 48))
    with pytest.raises(NotImplementedError):
        env.render('human')
    with pytest.raises(ValueError):
        plain.render('rgb_array')


def test_kilobots_env_rgb_array():
    from gym_kilobots_amd.envs.kilobots_env import KilobotsEnv
    from gym_kilobots_amd.lib.body import Quad
    from gym_kilobots_amd.lib.kilobot import SimpleVelocityControlKilobot
    from gym_kilobots_amd.lib.light import CircularGradientLight

    class Env(KilobotsEnv):
        screen_size = screen_width, screen_height = 600, 450        # (3.3 mm per pixel: no 5 mm mark slips between the pixel centres)

        def _configure_environment(self):
            self._light = CircularGradientLight(position=np.array([0.3, 0.2]), radius=0.15)
            box = Quad(world=self.world, width=0.2, height=0.1, position=(-0.3, 0.1), orientation=0.4)
            box.color = (250, 40, 10)
            self._add_object(box)
            for i in range(4):
                self._add_kilobot(SimpleVelocityControlKilobot(self.world, position=(0.1 * i - 0.1, -0.3), orientation=0.5 * i))
            self._kilobots[1].set_color((0, 200, 0))
            self._kilobots[2].set_color((0, 0, 220))
            self._kilobots[3]._highlight_color = (255, 0, 255)

        def get_reward(self, state, action, new_state):
            return 0.0

    assert 'rgb_array' in Env.metadata['render.modes']
    env = Env()
    env.reset()
    for mode in (None, 'human'):
        with pytest.raises(NotImplementedError):
            env.render(mode)
    frame = env.render('rgb_array')
    assert isinstance(frame, np.ndarray) and frame.dtype == np.uint8 and frame.shape == (450, 600, 3)
    kb = env.kilobots
    word = lambda c_: (int(c_[0]) << 16) | (int(c_[1]) << 8) | int(c_[2])
    body = np.array([[word(k._body_color) for k in kb]])
    mark = np.array([[word(k._highlight_color) for k in kb]])
    assert [tuple(k._body_color) for k in kb] == [(150, 150, 150), (0, 200, 0), (0, 0, 220), (150, 150, 150)]
    for col in ((0, 200, 0), (0, 0, 220), (255, 0, 255), (150, 150, 150)):
        assert (frame == np.array(col, dtype=np.uint8)).all(-1).any(), col
    assert (frame == np.array([250, 40, 10], dtype=np.uint8)).all(-1).sum() > 100
    w = want(env.sim, 600, 450, style=dict(obj=[(250, 40, 10)]), body=body, mark=mark)
    assert np.array_equal(frame, w[0])
    env.close()
