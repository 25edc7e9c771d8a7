#!/usr/bin/env python3
"""Times kb_sense_assign (KilobotSim.targets with match='greedy') at 4096 envs x 1024 kilobots, next to kb_sense_targets on the
same state -- the cost of its round 1 -- and to the loop it replaces, rounds of masked kb_sense_targets with the mask updates
in torch.

usage: tools/bench_assign.py [--envs 4096] [--bots 1024] [--slots 64,256,1024] [--launches 10] [--repeats 3] [--out FILE]

Two scenes, each against the square lattice of K slots of tools/bench_targets.py, shared by all envs: 'lattice', the settled
cfg3 scene of bench.py (every env its own jittered lattice, stepped --settle substeps), and 'cloud', a Gaussian cloud of
sigma = 0.1 m around the centre (positions only: nothing is stepped there, sensing does not mind overlaps).  Per scene and K:
kb_sense_assign with all five outputs and no cutoff; kb_sense_targets with all five outputs; R, the rounds the matching
takes (word 3 of the stats: mean and largest over the envs); and the loop: `rounds` times { kb_sense_targets over the entries
still unmatched, index and owner only; the pairs that name each other leave both masks }, with rounds = the largest R of the
batch taken from the stats beforehand, so that the loop needs no host sync to know when to stop -- a loop that asked the
device every round would be slower.  The kernel legs are timed alternately, `--repeats` times; every time is the mean over
`--launches` back-to-back calls between two device events after a warm-up of the same shape (the loop: `--loop-launches`); the
median is reported and all repeats kept beside it.  Checked outside the timed windows: the loop ends with the matching of the
kernel in every env, and env 0 equals the numpy restatement of the definition (tests/assign_ref.py) bit for bit when the
oracle library is there to give its sine and cosine.  KB_HIP_LIB selects another build of the library.  Prints one JSON line
(and writes it to --out)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--bots', type=int, default=1024)
    ap.add_argument('--slots', default='64,256,1024')
    ap.add_argument('--scenes', default='lattice,cloud')
    ap.add_argument('--tol', type=float, default=0.02)
    ap.add_argument('--sigma', type=float, default=0.1, help='of the cloud, metres')
    ap.add_argument('--launches', type=int, default=10)
    ap.add_argument('--loop-launches', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--no-loop', action='store_true', help='skip the torch loop')
    ap.add_argument('--settle', type=int, default=120, help='substeps before the state of the lattice scene is taken')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    import bench
    from bench_targets import lattice
    from gym_kilobots_amd import _native as nat
    from gym_kilobots_amd.sim import KilobotSim
    if not torch.cuda.is_available():
        sys.exit('bench_assign needs a GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    E, N = args.envs, args.bots
    sizes = [int(v) for v in args.slots.split(',')]

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

    def restated(sim, points, tol):
        """env 0 by the numpy restatement, or None where the oracle library cannot be built."""
        try:
            from tests import assign_ref
            cpu = lambda t: t[:1].cpu().numpy()
            return assign_ref.restate(cpu(sim.x), cpu(sim.y), cpu(sim.theta), points.cpu().numpy(), tol)
        except Exception as err:      # noqa: BLE001
            print('no restatement: %s' % err, file=sys.stderr)
            return None

    sim = KilobotSim(E, N, device=dev, allow_sleep=0)
    status = 0

    def place(scene):
        nonlocal status
        if scene == 'lattice':
            x, y, th, actions = bench.make_scene(torch, E, N, dev, args.seed, 0, 0)
            sim.x.copy_(x); sim.y.copy_(y); sim.theta.copy_(th)
            sim.forget_contacts()
            for s in range(args.settle):
                sim.step(1, actions=actions[s % len(actions)])
            torch.cuda.synchronize()
            status |= int(sim.status.max().item())
        else:
            g = torch.Generator(device=dev)
            g.manual_seed(7919 * (args.seed + 1))
            xy = torch.randn(E, N, 2, generator=g, device=dev, dtype=torch.float64) * args.sigma
            sim.x.copy_((xy[..., 0] * 25.0).float()); sim.y.copy_((xy[..., 1] * 25.0).float())
            sim.theta.copy_(((torch.rand(E, N, generator=g, device=dev, dtype=torch.float64) * 2.0 - 1.0) * np.pi).float())
            torch.cuda.synchronize()

    def loop(points, rounds, bots, slots, index, owner, match_b, match_s):
        """The loop kb_sense_assign replaces: per round one masked kb_sense_targets and the mask updates, all on the device."""
        K = points.shape[0]
        bots.fill_(1); slots.fill_(1); match_b.fill_(-1); match_s.fill_(-1)
        ar_b, ar_s = torch.arange(N, device=dev)[None], torch.arange(K, device=dev)[None]
        for _ in range(rounds):
            sim.targets(points, args.tol, bot_select=bots, slot_select=slots, rel=False, dist=False, stats=False, out=(index, owner))
            t, b = index.long().clamp_(min=0), owner.long().clamp_(min=0)
            mutual_b = (index >= 0) & (owner.gather(1, t) == ar_b)
            mutual_s = (owner >= 0) & (index.gather(1, b) == ar_s)
            torch.where(mutual_b, index, match_b, out=match_b)
            torch.where(mutual_s, owner, match_s, out=match_s)
            bots.masked_fill_(mutual_b, 0)
            slots.masked_fill_(mutual_s, 0)

    legs = []
    for scene in args.scenes.split(','):
        place(scene)
        for K in sizes:
            points = torch.from_numpy(lattice(K)).to(dev)
            index = torch.empty(E, N, dtype=torch.int32, device=dev)
            rel = torch.empty(E, N, 4, dtype=torch.float32, device=dev)
            owner = torch.empty(E, K, dtype=torch.int32, device=dev)
            dist = torch.empty(E, K, dtype=torch.float32, device=dev)
            stats = torch.empty(E, 6, dtype=torch.float32, device=dev)
            out = (index, rel, owner, dist, stats)
            t_assign, t_targets, t_loop = [], [], []
            for _ in range(args.repeats):
                t_assign.append(timed(lambda: sim.targets(points, args.tol, match='greedy', out=out), args.launches))
                t_targets.append(timed(lambda: sim.targets(points, args.tol, out=out), args.launches))
            sim.targets(points, args.tol, match='greedy', out=out)
            torch.cuda.synchronize()
            want = restated(sim, points, args.tol)
            same = None if want is None else bool(all(np.array_equal(t[0].cpu().numpy().view(np.uint32), w[0].view(np.uint32)) for t, w in zip(out, want)))
            assert same is not False, 'env 0 differs from the restatement'
            assert bool((stats[:, 5] == min(N, K)).all()) and int(index.max()) < K and int(owner.max()) < N
            rounds = int(stats[:, 3].max().item())
            a_ms, t_ms = float(np.median(t_assign)), float(np.median(t_targets))
            leg = {'scene': scene, 'slots': K, 'assign_ms': round(a_ms, 4), 'assign_ms_all': [round(v, 4) for v in t_assign],
                   'kb_sense_targets_ms': round(t_ms, 4), 'kb_sense_targets_ms_all': [round(v, 4) for v in t_targets],
                   'assign_over_targets': round(a_ms / t_ms, 2), 'rounds_mean': round(float(stats[:, 3].mean()), 2), 'rounds_max': rounds,
                   'mean_matched_distance_m': round(float((stats[:, 2] / stats[:, 5]).mean()), 5), 'env_0_equals_the_restatement': same}
            if not args.no_loop:
                bots, slots = torch.empty(E, N, dtype=torch.uint8, device=dev), torch.empty(E, K, dtype=torch.uint8, device=dev)
                l_index, l_owner = torch.empty_like(index), torch.empty_like(owner)
                match_b, match_s = torch.empty_like(index), torch.empty_like(owner)
                run = lambda: loop(points, rounds, bots, slots, l_index, l_owner, match_b, match_s)
                for _ in range(args.repeats):
                    t_loop.append(timed(run, args.loop_launches))
                torch.cuda.synchronize()
                assert torch.equal(match_b, index) and torch.equal(match_s, owner), 'the loop ends with another matching'
                l_ms = float(np.median(t_loop))
                leg.update({'loop_rounds': rounds, 'loop_ms': round(l_ms, 3), 'loop_ms_all': [round(v, 3) for v in t_loop], 'loop_over_assign': round(l_ms / a_ms, 2),
                            'loop_ends_with_the_same_matching': True})
                del bots, slots, l_index, l_owner, match_b, match_s
            legs.append(leg)
            print(json.dumps(leg), file=sys.stderr, flush=True)
            del index, rel, owner, dist, stats, out
            torch.cuda.empty_cache()
    line = {'metric': 'kb_sense_assign_ms', 'envs': E, 'bots': N, 'tol_m': args.tol, 'cloud_sigma_m': args.sigma, 'settle_substeps': args.settle,
            'launches_per_timing': args.launches, 'loop_launches_per_timing': args.loop_launches, 'repeats': args.repeats, 'status': status,
            'timer': 'device events around back-to-back calls, the kernel legs alternately, median of the repeats',
            'library': os.path.basename(nat.LIB_PATH), 'device': torch.cuda.get_device_name(0), 'legs': legs}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
