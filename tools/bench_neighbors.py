#!/usr/bin/env python3
"""Times kb_sense_neighbors on the settled cfg3 scene of bench.py (4096 envs x 1024 kilobots) next to two baselines.

usage: tools/bench_neighbors.py [--envs 4096] [--bots 1024] [--launches 50] [--repeats 3] [--out FILE]

Legs: (R, k) = (0.07, 8), (0.07, 16), (0.035, 4).  Baselines on the same poses and radius:
  kb_sense       the count alone: half the pairs, 4 B per kilobot (the nearest capability without the lists);
  torch          chunked torch.cdist + topk over the envs, what a user of poses() writes today (distances and indices only:
                 no range mask, no body frame, no count -- less than the kernel returns).
Every time is the mean over `--launches` back-to-back launches between two device events after a warm-up of the same
shape; the legs are interleaved and repeated `--repeats` times, the median is reported and the spread kept beside it.
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = [(0.07, 8), (0.07, 16), (0.035, 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--bots', type=int, default=1024)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--settle', type=int, default=120, help='substeps before the poses are taken')
    ap.add_argument('--chunk', type=int, default=64, help='envs per torch.cdist call (64 x 1024 x 1024 floats = 256 MiB)')
    ap.add_argument('--torch-passes', type=int, default=2)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    import bench
    from gym_kilobots_amd.sim import KilobotSim
    if not torch.cuda.is_available():
        sys.exit('bench_neighbors needs a GPU: a time taken anywhere else says nothing')
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

    def torch_topk(k):
        kk = min(k + 1, N)                      # (the nearest is the kilobot itself)
        for a in range(0, E, args.chunk):
            p = xy[a:a + args.chunk]
            d = torch.cdist(p, p)
            d.topk(kk, dim=-1, largest=False)

    legs = []
    for R, k in LEGS:
        out = tuple(torch.empty(*s, dtype=d, device=dev) for s, d in (((E, N, k), torch.int32), ((E, N, k, 4), torch.float32), ((E, N), torch.int32)))
        cnt = torch.empty(E, N, dtype=torch.int32, device=dev)
        t_nb, t_se, t_to = [], [], []
        for _ in range(args.repeats):
            t_nb.append(timed(lambda: sim.neighbors(R, k, out=out), args.launches))
            t_se.append(timed(lambda: sim.sense(R, out=cnt), args.launches))
            t_to.append(timed(lambda: torch_topk(k), args.torch_passes))
        assert torch.equal(out[2], cnt)
        ms, ms_sense, ms_torch = float(np.median(t_nb)), float(np.median(t_se)), float(np.median(t_to))
        out_bytes = E * N * (k * 20 + 4)
        gbs = out_bytes / (ms * 1e-3) / 1e9
        legs.append({'radius_m': R, 'k': k, 'ms': round(ms, 4), 'ms_all': [round(v, 4) for v in t_nb],
                     'kb_sense_ms': round(ms_sense, 4), 'kb_sense_ms_all': [round(v, 4) for v in t_se], 'ratio_to_kb_sense': round(ms / ms_sense, 3),
                     'torch_cdist_topk_ms': round(ms_torch, 3), 'torch_ms_all': [round(v, 3) for v in t_to], 'speedup_over_torch': round(ms_torch / ms, 1),
                     'output_bytes': out_bytes, 'output_gb_per_s': round(gbs, 1), 'hbm_roof_frac': round(gbs / bench.HBM_PEAK_GBS, 4),
                     'mean_in_range': round(float(cnt.float().mean().item()), 2), 'max_in_range': int(cnt.max().item())})
        del out
    line = {'metric': 'kb_sense_neighbors_ms', 'envs': E, 'bots': N, 'scene': 'cfg3 lattice after %d substeps' % args.settle,
            'launches_per_timing': args.launches, 'repeats': args.repeats, 'timer': 'device events around back-to-back launches, median of the repeats',
            'torch_baseline': 'torch.cdist + topk(k + 1, largest=False) in chunks of %d envs, %d passes per timing' % (args.chunk, args.torch_passes),
            'hbm_peak_gb_per_s': bench.HBM_PEAK_GBS, 'device': torch.cuda.get_device_name(0), 'legs': legs}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
