#!/usr/bin/env python3
"""Times kb_sense_grid on the settled cfg3 scene of bench.py (4096 envs x 1024 kilobots) and on its cfg4 variant with four
pushable discs, next to two baselines.

usage: tools/bench_grid.py [--envs 4096] [--bots 1024] [--launches 50] [--repeats 3] [--out FILE]

Grids 64 x 48 and 128 x 96; planes: the count alone and count + flow on both scenes, all three planes on the cfg4 scene
(the object planes need objects).  Baselines on the same state:
  kb_get_poses  the lightest launch that reads the same poses: 12 B in and 12 B out per kilobot.  kb_sense_grid reads 8 B per
                kilobot (12 with the flow) once per band and writes 4 C gw gh B per env;
  torch         the same definition (include/kilobots_hip.h) as a user of the state tensors would write it, in chunks of envs:
                cell indices with torch operations, scatter_add_ into int32 (the count; the rounded cosines and sines at
                scale 65536), and the object masks cell by cell on [chunk, gh, gw] tensors, geometry from kb_get_outline.
Every time is the mean over `--launches` back-to-back launches between two device events after a warm-up of the same
shape; the legs are interleaved and repeated `--repeats` times, the median is reported and all repeats kept beside it.
Checked on every leg, outside the timed windows: the count plane of the torch formulation equals the kernel's bit for bit
(the same fp32 operations in the same order).  torch's sine and cosine are not the library's, but both are within 2^-22 of
the exact ones, far less than half a unit of the fixed point: a kilobot's quantised value differs by at most one unit, so
a flow word may differ by at most count / 65536, and that is asserted cell by cell.  The object masks may differ only where
a rounding of the object's frame can move a cell centre across the outline: at cells next to the mask's edge; those cells
are counted into the line.
Prints one JSON line (and writes it to --out)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = [(64, 48), (128, 96)]


def constants(ol, gw, gh):
    """(xmin, ymin, cw, ch, icw, ich) as Python floats holding the fp32 values of the definition."""
    f = np.float32
    xmin, xmax, ymin, ymax = (f(v) for v in ol.arena)
    wx, wy = xmax - xmin, ymax - ymin
    return tuple(float(v) for v in (xmin, ymin, wx / f(gw), wy / f(gh), f(gw) / wx, f(gh) / wy))


def torch_grid(torch, nat, sim, ol, gw, gh, planes, out, chunk):
    """The definition in torch, every operation its own (unfused) tensor operation."""
    xmin, ymin, cw, ch, icw, ich = constants(ol, gw, gh)
    E, N = sim.x.shape
    dev = sim.x.device
    cells = gw * gh
    if planes & nat.GRID_OBJECTS:
        cx = (xmin + (torch.arange(gw, device=dev, dtype=torch.float32) + 0.5) * cw)[None, None, :]
        cy = (ymin + (torch.arange(gh, device=dev, dtype=torch.float32) + 0.5) * ch)[None, :, None]
    for a in range(0, E, chunk):
        sl = slice(a, min(a + chunk, E))
        n = sl.stop - sl.start
        c0 = 0
        if planes & (nat.GRID_COUNT | nat.GRID_FLOW):
            tx, ty = (sim.x[sl] - xmin) * icw, (sim.y[sl] - ymin) * ich
            zero = torch.zeros_like(tx, dtype=torch.int64)
            ix = torch.where(~(tx > 0), zero, torch.where(tx >= gw, zero + (gw - 1), tx.to(torch.int64)))
            iy = torch.where(~(ty > 0), zero, torch.where(ty >= gh, zero + (gh - 1), ty.to(torch.int64)))
            flat = ((torch.arange(n, device=dev)[:, None] * gh + iy) * gw + ix).view(-1)
            if planes & nat.GRID_COUNT:
                acc = torch.zeros(n * cells, dtype=torch.int32, device=dev)
                acc.scatter_add_(0, flat, torch.ones_like(flat, dtype=torch.int32))
                out[sl, c0] = acc.view(n, gh, gw).to(torch.float32)
                c0 += 1
            if planes & nat.GRID_FLOW:
                th = sim.theta[sl]
                for v in (torch.cos(th), torch.sin(th)):
                    q = torch.round(v * 65536.0).to(torch.int32).view(-1)     # (half to even; |v| <= 1: nothing to clamp)
                    acc = torch.zeros(n * cells, dtype=torch.int32, device=dev)
                    acc.scatter_add_(0, flat, q)
                    out[sl, c0] = acc.view(n, gh, gw).to(torch.float32) / 65536.0
                    c0 += 1
        if planes & nat.GRID_OBJECTS:
            for m in range(ol.num_objects):
                oth = sim.otheta[sl, m][:, None, None]
                so, co = torch.sin(oth), torch.cos(oth)
                dx, dy = cx - sim.ox[sl, m][:, None, None], cy - sim.oy[sl, m][:, None, None]
                px, py = co * dx + so * dy, co * dy - so * dx
                inside = torch.zeros_like(px, dtype=torch.bool)
                for f in range(ol.num_fixtures):
                    if ol.body[f] != m:
                        continue
                    nv = ol.nverts[f]
                    if nv == 0:
                        g = torch.sqrt(px * px + py * py) - float(ol.radius[f])
                        inside |= ~(g > 0)
                        continue
                    in_f = torch.ones_like(inside)
                    for k in range(nv):
                        ax, ay = np.float32(ol.verts[f][k][0]), np.float32(ol.verts[f][k][1])
                        bx, by = np.float32(ol.verts[f][(k + 1) % nv][0]), np.float32(ol.verts[f][(k + 1) % nv][1])
                        ex, ey = float(bx - ax), float(by - ay)
                        wx, wy = px - float(ax), py - float(ay)
                        in_f &= ex * wy - ey * wx >= 0
                    inside |= in_f
                out[sl, c0 + m] = inside.to(torch.float32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--bots', type=int, default=1024)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--settle', type=int, default=120, help='substeps before the state is taken')
    ap.add_argument('--chunk', type=int, default=512, help='envs per torch pass')
    ap.add_argument('--torch-passes', type=int, default=3)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F
    import bench
    from gym_kilobots_amd import _native as nat
    from gym_kilobots_amd.sim import KilobotSim
    if not torch.cuda.is_available():
        sys.exit('bench_grid needs a GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    E, N = args.envs, args.bots

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
    for name, M in (('cfg3: settled lattice', 0), ('cfg4: cfg3 + four discs', 4)):
        sim = KilobotSim(E, N, device=dev, num_objects=M, allow_sleep=0)
        x, y, th, actions = bench.make_scene(torch, E, N, dev, args.seed, 0, M)
        sim.x.copy_(x); sim.y.copy_(y); sim.theta.copy_(th)
        sim.forget_contacts()
        if M:
            sim.set_objects_m(np.tile(bench.CFG4_OBJECTS[None, :M], (E, 1, 1)))
        for s in range(args.settle):
            sim.step(1, actions=actions[s % len(actions)])
        torch.cuda.synchronize()
        status = int(sim.status.max().item())
        ol = sim.outline()
        poses = torch.empty(E, N, 3, dtype=torch.float32, device=dev)
        t_p = [timed(lambda: sim._lib.kb_get_poses(sim._h, C.c_void_p(poses.data_ptr()), sim._stream()), args.launches) for _ in range(args.repeats)]
        ms_p = float(np.median(t_p))
        del poses
        legs = []
        plane_sets = [('count', nat.GRID_COUNT), ('count + flow', nat.GRID_COUNT | nat.GRID_FLOW)]
        if M:
            plane_sets.append(('count + flow + objects', nat.GRID_COUNT | nat.GRID_FLOW | nat.GRID_OBJECTS))
        for gw, gh in GRIDS:
            for pname, planes in plane_sets:
                Cn = sim.grid_channels(planes)
                out = torch.empty(E, Cn, gh, gw, dtype=torch.float32, device=dev)
                ref = torch.empty_like(out)
                t_k, t_t = [], []
                for _ in range(args.repeats):
                    t_k.append(timed(lambda: sim.occupancy_grid(gw, gh, planes, out=out), args.launches))
                    t_t.append(timed(lambda: torch_grid(torch, nat, sim, ol, gw, gh, planes, ref, args.chunk), args.torch_passes))
                sim.occupancy_grid(gw, gh, planes, out=out)
                torch.cuda.synchronize()
                assert torch.equal(out[:, 0].contiguous().view(torch.int32), ref[:, 0].contiguous().view(torch.int32)), 'the count plane differs from the torch formulation'
                assert bool((out[:, 0].sum((1, 2)) == N).all())
                flow_units, mask_cells = 0, 0
                if planes & nat.GRID_FLOW:
                    err = (out[:, 1:3] - ref[:, 1:3]).abs() * 65536.0
                    assert bool((err <= out[:, :1]).all()), 'a flow word differs by more than one unit per kilobot of its cell'
                    flow_units = int(err.max().item())
                if planes & nat.GRID_OBJECTS:
                    mk, mt = out[:, 3:], ref[:, 3:]
                    edge = F.max_pool2d(mk, 3, 1, 1) != -F.max_pool2d(-mk, 3, 1, 1)
                    diff = mk != mt
                    assert not bool((diff & ~edge).any()), 'an object mask differs away from its edge'
                    assert bool((mk.amax((2, 3)) == 1).all()) and bool((mk.amin((2, 3)) == 0).all())
                    mask_cells = int(diff.sum().item())
                ms, ms_t = float(np.median(t_k)), float(np.median(t_t))
                out_bytes = out.numel() * 4
                gbs = out_bytes / (ms * 1e-3) / 1e9
                legs.append({'grid': [gw, gh], 'planes': pname, 'channels': Cn, 'ms': round(ms, 4), 'ms_all': [round(v, 4) for v in t_k],
                             'torch_ms': round(ms_t, 3), 'torch_ms_all': [round(v, 3) for v in t_t], 'speedup_over_torch': round(ms_t / ms, 1),
                             'ratio_to_kb_get_poses': round(ms / ms_p, 2), 'output_bytes': out_bytes, 'output_gb_per_s': round(gbs, 1),
                             'hbm_roof_frac': round(gbs / bench.HBM_PEAK_GBS, 4), 'largest_flow_difference_in_units_of_2^-16': flow_units,
                             'mask_cells_at_an_edge_where_torch_differs': mask_cells})
                del out, ref
                torch.cuda.empty_cache()
        scenes.append({'scene': name, 'objects': M, 'status': status, 'kb_get_poses_ms': round(ms_p, 4), 'kb_get_poses_ms_all': [round(v, 4) for v in t_p], 'legs': legs})
        sim.close()
        del sim
        torch.cuda.empty_cache()
    line = {'metric': 'kb_sense_grid_ms', 'envs': E, 'bots': N, 'settle_substeps': args.settle,
            'launches_per_timing': args.launches, 'repeats': args.repeats, 'timer': 'device events around back-to-back launches, median of the repeats',
            'torch_baseline': 'cell indices with torch operations, scatter_add_ into int32, object masks cell by cell on [chunk, gh, gw] tensors; '
                              'chunks of %d envs, %d passes per timing' % (args.chunk, args.torch_passes),
            'hbm_peak_gb_per_s': bench.HBM_PEAK_GBS, 'device': torch.cuda.get_device_name(0), 'scenes': scenes}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
