#!/usr/bin/env python3
"""Times kb_sense_hops on the settled cfg3 scene of bench.py (4096 envs x 1024 kilobots) next to the iteration it replaces.

usage: tools/bench_hops.py [--envs 4096] [--bots 1024] [--radii 0.05,0.07,0.1] [--launches 20] [--sweep-launches 3] [--repeats 10] [--out FILE]

Radii of 0.05, 0.07 and 0.1 m; two seed sets: kilobot 0 of every env, and a random 1 in 64.  Per (radius, seed set) four things
are timed alternately in the same process, `--repeats` times, each the mean over back-to-back calls between two device events
after a warm-up of the same shape; the median is reported and all repeats kept beside it:
  kb_sense_hops with hops alone, and with all four outputs (into preallocated tensors: the timed call is the one launch);
  the yardstick this entry replaces, on the same state: `deepest + 1` sweeps of h <- min(h, reduce_min(h) + 1), each a
    buf.copy_(h), a neighbor_reduce(op='min', out=buf) in place and a torch.minimum(h, buf + 1) -- as many sweeps as the
    deepest env of the batch needs to settle plus the one that would tell the caller so; `deepest` comes from the stats of
    kb_sense_hops, read outside the timed window (a caller without it has to guess higher);
  kb_sense_neighbors(R, 16), the common yardstick of the other sensing tools.
Checked outside the timed windows: env 0 equals the numpy restatement (tests/hops_ref.py), and the sweeps settle on the same
hop counts in every env.
Reported per leg: ms, deepest hop, mean frontier size (kilobots reached / levels, averaged over the envs), kilobots reached,
and the two ratios.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--bots', type=int, default=1024)
    ap.add_argument('--radii', default='0.05,0.07,0.1')
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--sweep-launches', type=int, default=3, help='runs of the whole reduce iteration per timing')
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--settle', type=int, default=120, help='substeps before the state is taken')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    import bench
    from gym_kilobots_amd import _native as nat
    from gym_kilobots_amd.sim import KilobotSim
    from tests import hops_ref
    if not torch.cuda.is_available():
        sys.exit('bench_hops needs a GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    E, N = args.envs, args.bots
    radii = [float(v) for v in args.radii.split(',')]

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

    sim = KilobotSim(E, N, device=dev, allow_sleep=0)
    x, y, th, actions = bench.make_scene(torch, E, N, dev, args.seed, 0, 0)
    sim.x.copy_(x); sim.y.copy_(y); sim.theta.copy_(th)
    sim.forget_contacts()
    for s in range(args.settle):
        sim.step(1, actions=actions[s % len(actions)])
    torch.cuda.synchronize()
    status = int(sim.status.max().item())
    first = torch.zeros(E, N, dtype=torch.bool, device=dev)
    first[:, 0] = True
    gen = torch.Generator(device='cpu').manual_seed(args.seed + 64)
    scattered = (torch.rand(E, N, generator=gen) < 1.0 / 64).to(dev)
    x0, y0 = sim.x[0].cpu().numpy(), sim.y[0].cpu().numpy()
    nbr = sim.neighbors(radii[0], 16)
    hops = torch.empty(E, N, dtype=torch.int32, device=dev)
    four = (hops.clone(), hops.clone(), hops.clone(), torch.empty(E, 2, dtype=torch.int32, device=dev))
    h0, h, buf = (torch.empty(E, N, dtype=torch.float32, device=dev) for _ in range(3))
    inf, minus = torch.full_like(h0, float('inf')), torch.full_like(h0, -1.0)
    legs = []
    for R in radii:
        for name, seeds in (('kilobot 0', first), ('random 1 in 64', scattered)):
            sim.hops(seeds, R, parent=True, root=True, stats=True, out=four)
            stats = four[3].cpu().numpy().astype(np.int64)
            deepest = int(stats[:, 1].max())
            seeded = stats[:, 1] >= 0
            want = hops_ref.restate_env(x0, y0, seeds[0].cpu().numpy(), R)
            same = bool(all(np.array_equal(t[0].cpu().numpy(), w) for t, w in zip(four, want)))
            assert same, 'env 0 differs from the restatement'
            torch.where(seeds, torch.zeros_like(h0), inf, out=h0)

            def sweeps():
                h.copy_(h0)
                for _ in range(deepest + 1):
                    buf.copy_(h)
                    sim.neighbor_reduce(buf, R, op='min', out=buf)
                    torch.minimum(h, buf + 1.0, out=h)
            t_h, t_4, t_s, t_n = [], [], [], []
            for _ in range(args.repeats):
                t_h.append(timed(lambda: sim.hops(seeds, R, out=hops), args.launches))
                t_4.append(timed(lambda: sim.hops(seeds, R, parent=True, root=True, stats=True, out=four), args.launches))
                t_s.append(timed(sweeps, args.sweep_launches))
                t_n.append(timed(lambda: sim.neighbors(R, 16, out=nbr), args.launches))
            torch.cuda.synchronize()
            settled = bool(torch.equal(torch.where(torch.isinf(h), minus, h).to(torch.int32), hops)) and bool(torch.equal(hops, four[0]))
            assert settled, 'the reduce iteration and kb_sense_hops disagree'
            ms, ms4, ms_s, ms_n = (float(np.median(t)) for t in (t_h, t_4, t_s, t_n))
            levels = stats[seeded, 1] + 1
            legs.append({'radius_m': R, 'seeds': name, 'seeds_per_env': round(float(seeds.sum().item()) / E, 3),
                         'ms': round(ms, 4), 'ms_all': [round(v, 4) for v in t_h],
                         'all_four_outputs_ms': round(ms4, 4), 'all_four_outputs_ms_all': [round(v, 4) for v in t_4],
                         'deepest_hop': deepest, 'mean_deepest_hop': round(float(stats[seeded, 1].mean()), 2),
                         'mean_frontier': round(float((stats[seeded, 0] / levels).mean()), 2),
                         'reached_per_env': round(float(stats[:, 0].mean()), 2), 'envs_without_a_seed': int((~seeded).sum()),
                         'reduce_sweeps': deepest + 1, 'reduce_sweeps_ms': round(ms_s, 4), 'reduce_sweeps_ms_all': [round(v, 4) for v in t_s],
                         'ratio_to_reduce_sweeps': round(ms / ms_s, 4), 'all_four_ratio_to_reduce_sweeps': round(ms4 / ms_s, 4),
                         'faster_than_the_sweeps': bool(ms < ms_s and ms4 < ms_s),
                         'kb_sense_neighbors_16_ms': round(ms_n, 4), 'kb_sense_neighbors_16_ms_all': [round(v, 4) for v in t_n],
                         'ratio_to_kb_sense_neighbors': round(ms / ms_n, 3),
                         'env_0_equals_the_restatement': same, 'sweeps_settle_on_the_same_hops': settled})
    line = {'metric': 'kb_sense_hops_ms', 'envs': E, 'bots': N, 'scene': 'cfg3: settled lattice', 'status': status, 'settle_substeps': args.settle,
            'launches_per_timing': args.launches, 'sweep_runs_per_timing': args.sweep_launches, 'repeats': args.repeats,
            'timer': 'device events around back-to-back calls; hops alone, all four outputs, the reduce iteration and kb_sense_neighbors alternately, median of the repeats',
            'library': os.path.basename(nat.LIB_PATH), 'device': torch.cuda.get_device_name(0), 'legs': legs}
    sim.close()
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
