#!/usr/bin/env python3
"""Times kb_sense_objects on the settled cfg4 scene of bench.py (4096 envs x 1024 kilobots, four discs), then on its four-box
variant, next to two baselines.

usage: tools/bench_objects.py [--envs 4096] [--bots 1024] [--launches 50] [--repeats 3] [--out FILE]

Baselines on the same state:
  kb_get_poses  the lightest launch that reads the same poses: 12 B in and 12 B out per kilobot.  kb_sense_objects reads the
                same 12 B and writes 16 (M + 1) B per kilobot; if it is bound by its output it sits near kb_get_poses scaled by
                the bytes written (`ratio_to_kb_get_poses` next to `output_bytes_ratio`);
  torch         a restatement of the same definition (include/kilobots_hip.h) a user of the state tensors would write, in
                chunks of envs, object by object and edge by edge on [chunk, N] tensors, geometry from kb_get_outline.
Every time is the mean over `--launches` back-to-back launches between two device events after a warm-up of the same
shape; the legs are interleaved and repeated `--repeats` times, the median is reported and all repeats kept beside it.
Checked on every scene, outside the timed windows: where torch's operations are the library's in the same order -- the wall
index and the signed wall distance, which involve no sine or cosine -- the restatement must equal the kernel bit for bit.
Elsewhere (torch's sine and cosine are not the library's) the kernel is compared with the restatement evaluated in float64:
distances and wall points within the rounding bound of tests/test_objects_cpu.py (1.95e-5 m) at EVERY kilobot; object points
within it at every row but those where the float64 evaluation itself shows two candidates within two bounds of each other
(the two evaluations may pick different ones): those rows are counted into the line; the inside flag may differ only
within the bound of the outline.
Prints one JSON line (and writes it to --out)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOUND_WU = (40 * 2.0 ** -24 + 6 * 2.0 ** -22) * 128.0      # tests/test_objects_cpu.py derives it
BOUND_M = BOUND_WU / 25.0


def torch_points(torch, sim, ol, dt, obj, wall, chunk, second=None):
    """The definition in torch on tensors of dtype dt, every operation its own (unfused) tensor operation, divisions
    tensor by tensor (torch multiplies by the reciprocal for tensor / scalar).  second (optional, [E, N, M]): the
    distance in world units of the best candidate that did not win."""
    for a in range(0, sim.x.shape[0], chunk):
        sl = slice(a, a + chunk)
        x, y, th = sim.x[sl].to(dt), sim.y[sl].to(dt), sim.theta[sl].to(dt)
        si, ci = torch.sin(th), torch.cos(th)
        S = torch.full_like(x, 25.0)
        zero = torch.zeros_like(x)
        for m in range(ol.num_objects):
            oth = sim.otheta[sl, m:m + 1].to(dt)
            so, co = torch.sin(oth), torch.cos(oth)
            dx, dy = x - sim.ox[sl, m:m + 1].to(dt), y - sim.oy[sl, m:m + 1].to(dt)
            px, py = co * dx + so * dy, co * dy - so * dx
            best, sec = torch.full_like(x, float('inf')), torch.full_like(x, float('inf'))
            brx, bry = zero, zero
            inside = torch.zeros_like(x, dtype=torch.bool)
            for f in range(ol.num_fixtures):
                if ol.body[f] != m:
                    continue
                n = ol.nverts[f]
                if n == 0:
                    r = float(ol.radius[f])
                    nn = torch.sqrt(px * px + py * py)
                    g = nn - r
                    pos = nn > 0
                    cand = [(g * g, torch.where(pos, -(g * (px / nn)), torch.full_like(x, r)), torch.where(pos, -(g * (py / nn)), zero))]
                    inside |= ~(g > 0)
                else:
                    cand, in_f = [], torch.ones_like(inside)
                    for k in range(n):
                        ax, ay = float(ol.verts[f][k][0]), float(ol.verts[f][k][1])
                        bx, by = float(ol.verts[f][(k + 1) % n][0]), float(ol.verts[f][(k + 1) % n][1])
                        ft = np.float32 if dt == torch.float32 else np.float64      # (the edge and its square in the precision of the pass)
                        ex, ey = ft(bx) - ft(ax), ft(by) - ft(ay)
                        ex, ey, den = float(ex), float(ey), float(ex * ex + ey * ey)
                        wx, wy = px - ax, py - ay
                        t = (wx * ex + wy * ey) / torch.full_like(x, den)
                        lo, hi = ~(t > 0), t >= 1
                        qx = torch.where(lo, torch.full_like(x, ax), torch.where(hi, torch.full_like(x, bx), ax + t * ex))
                        qy = torch.where(lo, torch.full_like(x, ay), torch.where(hi, torch.full_like(x, by), ay + t * ey))
                        rx, ry = qx - px, qy - py
                        cand.append((rx * rx + ry * ry, rx, ry))
                        in_f &= ex * wy - ey * wx >= 0
                    inside |= in_f
                for d2, rx, ry in cand:
                    better = d2 < best
                    if second is not None:
                        sec = torch.where(better, best, torch.minimum(sec, d2))
                    brx, bry, best = torch.where(better, rx, brx), torch.where(better, ry, bry), torch.where(better, d2, best)
            gx, gy = co * brx - so * bry, so * brx + co * bry
            obj[sl, :, m, 0] = (ci * gx + si * gy) / S
            obj[sl, :, m, 1] = (ci * gy - si * gx) / S
            obj[sl, :, m, 2] = torch.sqrt(best) / S
            obj[sl, :, m, 3] = inside.to(dt)
            if second is not None:
                second[sl, :, m] = torch.sqrt(sec)
        g0, g1, g2, g3 = x - float(ol.arena[0]), float(ol.arena[1]) - x, y - float(ol.arena[2]), float(ol.arena[3]) - y
        g, gx, gy, w = g0, -g0, zero, zero
        for idx, (gk, vx, vy) in enumerate(((g1, g1, zero), (g2, zero, -g2), (g3, zero, g3)), start=1):
            less = gk < g
            g, gx, gy, w = torch.where(less, gk, g), torch.where(less, vx, gx), torch.where(less, vy, gy), torch.where(less, torch.full_like(x, float(idx)), w)
        wall[sl, :, 0] = (ci * gx + si * gy) / S
        wall[sl, :, 1] = (ci * gy - si * gx) / S
        wall[sl, :, 2] = g / S
        wall[sl, :, 3] = w
    return obj, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--bots', type=int, default=1024)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--settle', type=int, default=120, help='substeps before the state is taken')
    ap.add_argument('--chunk', type=int, default=512, help='envs per torch pass')
    ap.add_argument('--torch-passes', type=int, default=1)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    import bench
    from gym_kilobots_amd.sim import KilobotSim
    if not torch.cuda.is_available():
        sys.exit('bench_objects needs a GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    E, N, M = args.envs, args.bots, 4

    def timed(fn, n):
        fn()                                    # warm-up of this shape
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(n):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / n          # ms per call

    scenes = []
    for name, okw in (('cfg4: four discs', {}),
                      ('cfg4: four boxes', dict(obj_shape=[1] * M, obj_nverts=[4] * M, obj_verts=[[[0.075 * 25.0, 0.075 * 25.0]]] * M))):
        sim = KilobotSim(E, N, device=dev, num_objects=M, allow_sleep=0, **okw)
        x, y, th, actions = bench.make_scene(torch, E, N, dev, args.seed, 0, M)
        sim.x.copy_(x); sim.y.copy_(y); sim.theta.copy_(th)
        sim.forget_contacts()
        sim.set_objects_m(np.tile(bench.CFG4_OBJECTS[None, :M], (E, 1, 1)))
        for s in range(args.settle):
            sim.step(1, actions=actions[s % len(actions)])
        torch.cuda.synchronize()
        status = int(sim.status.max().item())
        ol = sim.outline()
        obj = torch.empty(E, N, M, 4, dtype=torch.float32, device=dev)
        wall = torch.empty(E, N, 4, dtype=torch.float32, device=dev)
        poses = torch.empty(E, N, 3, dtype=torch.float32, device=dev)
        t_obj, t_wall = torch.empty_like(obj), torch.empty_like(wall)
        t_k, t_w, t_p, t_t = [], [], [], []
        for _ in range(args.repeats):
            t_k.append(timed(lambda: sim.object_points(out=(obj, wall)), args.launches))
            t_w.append(timed(lambda: sim._lib.kb_sense_objects(sim._h, None, C.c_void_p(wall.data_ptr()), sim._stream()), args.launches))
            t_p.append(timed(lambda: sim._lib.kb_get_poses(sim._h, C.c_void_p(poses.data_ptr()), sim._stream()), args.launches))
            t_t.append(timed(lambda: torch_points(torch, sim, ol, torch.float32, t_obj, t_wall, args.chunk), args.torch_passes))
        sim.object_points(out=(obj, wall))
        torch.cuda.synchronize()
        # where torch's op order is the library's: bit for bit
        assert torch.equal(t_wall[..., 2:].contiguous().view(torch.int32), wall[..., 2:].contiguous().view(torch.int32)), 'wall distance / index differ from the torch restatement'
        del t_obj, t_wall, poses
        # elsewhere: against float64, within the derived bound
        obj64 = torch.empty(E, N, M, 4, dtype=torch.float64, device=dev)
        wall64 = torch.empty(E, N, 4, dtype=torch.float64, device=dev)
        second = torch.empty(E, N, M, dtype=torch.float64, device=dev)
        torch_points(torch, sim, ol, torch.float64, obj64, wall64, args.chunk, second)
        derr = (obj[..., 2].double() - obj64[..., 2]).abs()
        verr = (obj[..., :2].double() - obj64[..., :2]).abs().amax(-1)
        werr = (wall[..., :3].double() - wall64[..., :3]).abs().amax(-1)
        assert float(derr.max()) <= BOUND_M, 'distance misses the bound: %g' % float(derr.max())
        assert float(werr.max()) <= BOUND_M and torch.equal(wall[..., 3].double(), wall64[..., 3]), 'wall point misses the bound: %g' % float(werr.max())
        far = verr > BOUND_M
        margin = second - obj64[..., 2] * 25.0
        assert bool((margin[far] <= 2 * BOUND_WU).all()), 'an object point misses the bound away from a tie'
        flip = obj[..., 3].double() != obj64[..., 3]
        assert bool((obj64[..., 2][flip] <= BOUND_M).all()), 'the inside flag differs away from the outline'
        ms, ms_w, ms_p, ms_t = (float(np.median(v)) for v in (t_k, t_w, t_p, t_t))
        out_bytes, poses_bytes = E * N * 16 * (M + 1), E * N * 12
        gbs = out_bytes / (ms * 1e-3) / 1e9
        scenes.append({'scene': name, 'objects': M, 'fixtures': ol.num_fixtures, 'status': status,
                       'ms': round(ms, 4), 'ms_all': [round(v, 4) for v in t_k],
                       'walls_only_ms': round(ms_w, 4), 'walls_only_ms_all': [round(v, 4) for v in t_w],
                       'kb_get_poses_ms': round(ms_p, 4), 'kb_get_poses_ms_all': [round(v, 4) for v in t_p],
                       'ratio_to_kb_get_poses': round(ms / ms_p, 2), 'output_bytes_ratio': round(out_bytes / poses_bytes, 2),
                       'torch_ms': round(ms_t, 3), 'torch_ms_all': [round(v, 3) for v in t_t], 'speedup_over_torch': round(ms_t / ms, 1),
                       'output_bytes': out_bytes, 'output_gb_per_s': round(gbs, 1), 'hbm_roof_frac': round(gbs / bench.HBM_PEAK_GBS, 4),
                       'rows_inside': int(obj[..., 3].sum().item()), 'largest_distance_error_m': float(derr.max()), 'largest_wall_error_m': float(werr.max()),
                       'rows_near_a_tie_where_the_point_differs': int(far.sum().item()), 'rows_where_the_inside_flag_differs': int(flip.sum().item()), 'bound_m': BOUND_M})
        del sim, obj, wall, obj64, wall64, second
        torch.cuda.empty_cache()
    line = {'metric': 'kb_sense_objects_ms', 'envs': E, 'bots': N, 'settle_substeps': args.settle,
            'launches_per_timing': args.launches, 'repeats': args.repeats, 'timer': 'device events around back-to-back launches, median of the repeats',
            'torch_baseline': 'the definition object by object and edge by edge on [chunk, N] tensors, chunks of %d envs, %d passes per timing' % (args.chunk, args.torch_passes),
            'hbm_peak_gb_per_s': bench.HBM_PEAK_GBS, 'device': torch.cuda.get_device_name(0), 'scenes': scenes}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
