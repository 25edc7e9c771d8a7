#!/usr/bin/env python3
"""Times kb_sense_clusters on the settled cfg3 scene of bench.py (4096 envs x 1024 kilobots) and on a Gaussian cloud, next to
the loop it replaces.

usage: tools/bench_clusters.py [--envs 4096] [--bots 1024] [--radii 0.05,0.07,0.1] [--launches 20] [--repeats 7] [--loop-repeats 2] [--out FILE]

Two scenes: the lattice of bench.py after `--settle` substeps, and the spawn of kb_reset with a standard deviation of
`--cloud-std` metres and no step to resolve (a cloud that thins out into isolated kilobots).  Radii of 0.05, 0.07 and 0.1 m.
Per (scene, radius) five things are timed alternately in the same process on the same state, each the mean over
back-to-back calls between two device events after a warm-up of the same shape; the median of `--repeats` is reported and
all repeats kept beside it:
  kb_sense_clusters with the label alone, and with all four outputs (into preallocated tensors: the timed call is the one launch);
  kb_sense at the same radius: one stencil walk and nothing else, the floor;
  one kb_sense_hops from kilobot 0 of every env (hops and root);
  the path this entry replaces: hops() seeded at the lowest kilobot of every env that has no label yet, root into label, until
    every kilobot of every env has one -- one launch, a handful of small torch kernels and one host decision per round, as
    many rounds as the env with the most components has components; timed `--loop-repeats` times as a whole, its launches
    reported, its result checked equal to the label of kb_sense_clusters.
Checked outside the timed windows: env 0 equals the numpy restatement (tests/clusters_ref.py), all four outputs.
Prints one JSON line (and writes it to --out)."""
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
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--loop-repeats', type=int, default=2, help='runs of the whole replaced loop per leg')
    ap.add_argument('--settle', type=int, default=120, help='substeps before the state of the lattice scene is taken')
    ap.add_argument('--cloud-std', type=float, default=0.3, help='standard deviation of the Gaussian cloud in metres')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    import bench
    from gym_kilobots_amd import _native as nat
    from gym_kilobots_amd.sim import KilobotSim
    from tests import clusters_ref
    if not torch.cuda.is_available():
        sys.exit('bench_clusters needs a GPU: a time taken anywhere else says nothing')
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
    label = torch.empty(E, N, dtype=torch.int32, device=dev)
    four = (label.clone(), label.clone(), torch.empty(E, N, 4, dtype=torch.float32, device=dev), torch.empty(E, 4, dtype=torch.int32, device=dev))
    count = torch.empty(E, N, dtype=torch.int32, device=dev)
    hops, root, loop_label = label.clone(), label.clone(), label.clone()
    first = torch.zeros(E, N, dtype=torch.bool, device=dev)
    first[:, 0] = True
    seeds = torch.zeros(E, N, dtype=torch.bool, device=dev)
    envs = torch.arange(E, device=dev)
    minus = torch.full_like(label, -1)

    def replaced_loop(R):
        """label by hops() from the lowest unlabelled kilobot of every env, until none is left; returns the launches"""
        loop_label.copy_(minus)
        launches = 0
        while True:
            open_ = loop_label < 0
            has = open_.any(1)
            if not bool(has.any()):             # the host decision of every round
                return launches
            lowest = open_.to(torch.int8).argmax(1)
            seeds.zero_()
            seeds[envs[has], lowest[has]] = True
            sim.hops(seeds, R, root=True, out=(hops, root))
            torch.where(open_ & (root >= 0), root, loop_label, out=loop_label)
            launches += 1

    legs = []
    for scene in ('cfg3: settled lattice', 'gaussian cloud'):
        if scene == 'gaussian cloud':
            sim.reset(seed=args.seed + 1, std=args.cloud_std, resolve=False)
        else:
            x, y, th, actions = bench.make_scene(torch, E, N, dev, args.seed, 0, 0)
            sim.x.copy_(x); sim.y.copy_(y); sim.theta.copy_(th)
            sim.forget_contacts()
            for s in range(args.settle):
                sim.step(1, actions=actions[s % len(actions)])
        torch.cuda.synchronize()
        status = int(sim.status.max().item())
        x0, y0 = sim.x[0].cpu().numpy(), sim.y[0].cpu().numpy()
        for R in radii:
            sim.clusters(R, size=True, table=True, stats=True, out=four)
            stats = four[3].cpu().numpy().astype(np.int64)
            want = clusters_ref.restate_env(x0, y0, R)
            same = bool(all(np.array_equal(t[0].cpu().numpy().view(np.int32), np.ascontiguousarray(w).view(np.int32)) for t, w in zip(four, want)))
            assert same, 'env 0 differs from the restatement'
            t_l, t_4, t_s, t_h, t_loop = [], [], [], [], []
            for _ in range(args.repeats):
                t_l.append(timed(lambda: sim.clusters(R, out=label), args.launches))
                t_4.append(timed(lambda: sim.clusters(R, size=True, table=True, stats=True, out=four), args.launches))
                t_s.append(timed(lambda: sim.sense(R, out=count), args.launches))
                t_h.append(timed(lambda: sim.hops(first, R, root=True, out=(hops, root)), args.launches))
            launches = replaced_loop(R)         # warm-up of the whole loop, and its check
            agree = bool(torch.equal(loop_label, label)) and bool(torch.equal(label, four[0]))
            assert agree, 'the hops loop and kb_sense_clusters disagree'
            for _ in range(args.loop_repeats):
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                replaced_loop(R)
                t1.record()
                t1.synchronize()
                t_loop.append(t0.elapsed_time(t1))
            ms, ms4, ms_s, ms_h, ms_loop = (float(np.median(t)) for t in (t_l, t_4, t_s, t_h, t_loop))
            legs.append({'scene': scene, 'radius_m': R, 'status': status,
                         'ms': round(ms, 4), 'ms_all': [round(v, 4) for v in t_l],
                         'all_four_outputs_ms': round(ms4, 4), 'all_four_outputs_ms_all': [round(v, 4) for v in t_4],
                         'components_per_env_mean': round(float(stats[:, 0].mean()), 2), 'components_per_env_max': int(stats[:, 0].max()),
                         'largest_per_env_mean': round(float(stats[:, 1].mean()), 2), 'isolated_per_env_mean': round(float(stats[:, 3].mean()), 2),
                         'kb_sense_ms': round(ms_s, 4), 'kb_sense_ms_all': [round(v, 4) for v in t_s], 'ratio_to_kb_sense': round(ms / ms_s, 3),
                         'one_kb_sense_hops_ms': round(ms_h, 4), 'one_kb_sense_hops_ms_all': [round(v, 4) for v in t_h],
                         'ratio_to_one_kb_sense_hops': round(ms / ms_h, 3),
                         'hops_loop_launches': launches, 'hops_loop_ms': round(ms_loop, 4), 'hops_loop_ms_all': [round(v, 4) for v in t_loop],
                         'ratio_to_hops_loop': round(ms / ms_loop, 4), 'all_four_ratio_to_hops_loop': round(ms4 / ms_loop, 4),
                         'faster_than_the_hops_loop': bool(ms < ms_loop and ms4 < ms_loop),
                         'env_0_equals_the_restatement': same, 'hops_loop_gives_the_same_label': agree})
    line = {'metric': 'kb_sense_clusters_ms', 'envs': E, 'bots': N, 'settle_substeps': args.settle, 'cloud_std_m': args.cloud_std,
            'launches_per_timing': args.launches, 'repeats': args.repeats, 'loop_repeats': args.loop_repeats,
            'timer': 'device events around back-to-back calls; label alone, all four outputs, kb_sense and one kb_sense_hops alternately, median of the repeats; the hops loop as a whole, host decisions included',
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
