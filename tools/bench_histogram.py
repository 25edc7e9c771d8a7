#!/usr/bin/env python3
"""Times kb_sense_histogram on the settled cfg3 scene of bench.py (4096 envs x 1024 kilobots) next to three baselines.

usage: tools/bench_histogram.py [--envs 4096] [--bots 1024] [--launches 50] [--repeats 3] [--out FILE]

Legs: (R, rings, sectors) = (0.07, 4, 8), (0.07, 8, 8), (0.15, 4, 8).  Baselines on the same poses and radius:
  kb_sense            the count alone: the same walk over half the stencil, 4 B per kilobot -- a lower bound;
  kb_sense_neighbors  the 16 nearest with their body-frame offsets (what the histogram replaces in dense scenes);
  torch               a chunked restatement a user of poses() would write: cdist -> range mask, ring from the distance,
                      sector from atan2 in the body frame -> scatter_add into [E, N, B] (its boundary cases are not the
                      library's; its totals are compared with the kernel's counts).
Every time is the mean over `--launches` back-to-back launches between two device events after a warm-up of the same
shape; the legs are interleaved and repeated `--repeats` times, the median is reported and the spread kept beside it.
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = [(0.07, 4, 8), (0.07, 8, 8), (0.15, 4, 8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--bots', type=int, default=1024)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--settle', type=int, default=120, help='substeps before the poses are taken')
    ap.add_argument('--chunk', type=int, default=32, help='envs per torch pass (32 x 1024 x 1024 floats = 128 MiB per temporary)')
    ap.add_argument('--torch-passes', type=int, default=1)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    import bench
    from gym_kilobots_amd.sim import KilobotSim
    if not torch.cuda.is_available():
        sys.exit('bench_histogram needs a GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    E, N = args.envs, args.bots
    sim = KilobotSim(E, N, device=dev, allow_sleep=0)
    x, y, th, actions = bench.make_scene(torch, E, N, dev, args.seed, 0, 0)
    sim.x.copy_(x); sim.y.copy_(y); sim.theta.copy_(th)
    sim.forget_contacts()
    for s in range(args.settle):
        sim.step(1, actions=actions[s % len(actions)])
    torch.cuda.synchronize()
    assert int(sim.status.max().item()) == 0

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

    poses = sim.poses()
    xy = poses[..., :2].contiguous()
    heading = poses[..., 2].contiguous()
    eye = torch.eye(N, dtype=torch.bool, device=dev)

    def torch_hist(R, rings, sectors, out):
        B = rings * sectors
        for a in range(0, E, args.chunk):
            p, t = xy[a:a + args.chunk], heading[a:a + args.chunk]
            d = torch.cdist(p, p)
            inr = (d <= R) & ~eye
            ring = torch.clamp(torch.ceil(d * (rings / R)) - 1, 0, rings - 1).long()
            ex = p[:, None, :, 0] - p[:, :, None, 0]
            ey = p[:, None, :, 1] - p[:, :, None, 1]
            bearing = torch.remainder(torch.atan2(ey, ex) - t[:, :, None], 2 * math.pi)
            sector = torch.clamp(torch.floor(bearing * (sectors / (2 * math.pi))), 0, sectors - 1).long()
            out[a:a + args.chunk].zero_().scatter_add_(2, ring * sectors + sector, inr.float())
        return out

    legs = []
    for R, rings, sectors in LEGS:
        B = rings * sectors
        hist = torch.empty(E, N, rings, sectors, dtype=torch.float32, device=dev)
        cnt = torch.empty(E, N, dtype=torch.int32, device=dev)
        hcnt = torch.empty(E, N, dtype=torch.int32, device=dev)
        nb = tuple(torch.empty(*s, dtype=d, device=dev) for s, d in (((E, N, 16), torch.int32), ((E, N, 16, 4), torch.float32), ((E, N), torch.int32)))
        th_out = torch.empty(E, N, B, dtype=torch.float32, device=dev)
        t_h, t_se, t_nb, t_to = [], [], [], []
        for _ in range(args.repeats):
            t_h.append(timed(lambda: sim.neighbor_histogram(R, rings, sectors, out=hist), args.launches))
            t_se.append(timed(lambda: sim.sense(R, out=cnt), args.launches))
            t_nb.append(timed(lambda: sim.neighbors(R, 16, out=nb), args.launches))
            t_to.append(timed(lambda: torch_hist(R, rings, sectors, th_out), args.torch_passes))
        sim.neighbor_histogram(R, rings, sectors, out=(hist, hcnt), count=True)
        assert torch.equal(hcnt, cnt) and torch.equal(nb[2], cnt)
        assert torch.equal(hist.sum((2, 3)), cnt.float())
        # the torch restatement rounds differently at the rim and at the bin boundaries: report how far apart the two are
        torch_in_range = float(th_out.sum().item())
        bins_differ = int((th_out.view_as(hist) != hist).sum().item())
        ms, ms_sense, ms_nb, ms_torch = (float(np.median(v)) for v in (t_h, t_se, t_nb, t_to))
        out_bytes = E * N * B * 4
        gbs = out_bytes / (ms * 1e-3) / 1e9
        legs.append({'radius_m': R, 'n_rings': rings, 'n_sectors': sectors, 'ms': round(ms, 4), 'ms_all': [round(v, 4) for v in t_h],
                     'kb_sense_ms': round(ms_sense, 4), 'kb_sense_ms_all': [round(v, 4) for v in t_se], 'ratio_to_kb_sense': round(ms / ms_sense, 3),
                     'kb_sense_neighbors_16_ms': round(ms_nb, 4), 'kb_sense_neighbors_ms_all': [round(v, 4) for v in t_nb],
                     'ratio_to_kb_sense_neighbors': round(ms / ms_nb, 3),
                     'torch_ms': round(ms_torch, 3), 'torch_ms_all': [round(v, 3) for v in t_to], 'speedup_over_torch': round(ms_torch / ms, 1),
                     'output_bytes': out_bytes, 'output_gb_per_s': round(gbs, 1), 'hbm_roof_frac': round(gbs / bench.HBM_PEAK_GBS, 4),
                     'mean_in_range': round(float(cnt.float().mean().item()), 2), 'max_in_range': int(cnt.max().item()),
                     'torch_total_in_range': torch_in_range, 'kernel_total_in_range': float(cnt.sum().item()),
                     'bins_where_torch_differs': bins_differ})
        del hist, nb, th_out
    line = {'metric': 'kb_sense_histogram_ms', 'envs': E, 'bots': N, 'scene': 'cfg3 lattice after %d substeps' % args.settle,
            'launches_per_timing': args.launches, 'repeats': args.repeats, 'timer': 'device events around back-to-back launches, median of the repeats',
            'torch_baseline': 'torch.cdist -> masks, ceil ring, atan2 sector -> scatter_add in chunks of %d envs, %d passes per timing' % (args.chunk, args.torch_passes),
            'hbm_peak_gb_per_s': bench.HBM_PEAK_GBS, 'device': torch.cuda.get_device_name(0), 'legs': legs}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
