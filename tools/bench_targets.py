#!/usr/bin/env python3
"""Times kb_sense_targets on the settled cfg3 scene of bench.py (4096 envs x 1024 kilobots), next to kb_sense_coverage at
64 x 48 on the same state and to the torch formulation it replaces.

usage: tools/bench_targets.py [--envs 4096] [--bots 1024] [--slots 64,256,1024] [--launches 20] [--repeats 3] [--out FILE]

Per K: the slots are a square lattice of K points over the middle 1.6 x 1.2 m of the table, shared by all envs;
kb_sense_targets with all five outputs, and with d_index and d_rel alone (the kilobot-to-slot direction and, for mutual, the
other one); (a) kb_sense_coverage at 64 x 48 with all four outputs, the one-sided nearest query on a regular grid; (b) torch on
the same state: broadcast squared distances [envs, kilobots, slots], min / argmin over the slots and over the kilobots, in
chunks of envs that fit `--chunk-mib` of memory per temporary (index, owner and the two distances only: no frame, no mutual,
no stats).  The kernel legs are timed alternately, `--repeats` times; every time is the mean over `--launches` back-to-back
calls between two device events after a warm-up of the same shape (the torch leg: `--torch-launches`); the median is reported
and all repeats kept beside it.  Checked outside the timed windows: env 0 equals the numpy restatement of the definition
(tests/targets_ref.py) bit for bit when the oracle library is there to give its sine and cosine; the share of kilobots and
slots on which torch names the same partner is reported (it may round d2 otherwise and breaks ties its own way).
KB_HIP_LIB selects another build of the library.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lattice(K, width=1.6, height=1.2):
    """K points [K, 2] float32 in metres: the first K of a square lattice over width x height around the centre."""
    side = int(np.ceil(np.sqrt(K)))
    i = np.arange(K)
    return np.stack([((i % side) + 0.5) / side * width - width / 2, ((i // side) + 0.5) / side * height - height / 2], -1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--bots', type=int, default=1024)
    ap.add_argument('--slots', default='64,256,1024')
    ap.add_argument('--tol', type=float, default=0.02)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--torch-launches', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--chunk-mib', type=int, default=512)
    ap.add_argument('--no-torch', action='store_true', help='skip leg (b)')
    ap.add_argument('--settle', type=int, default=120, help='substeps before the state is taken')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    import bench
    from gym_kilobots_amd import _native as nat
    from gym_kilobots_amd.sim import KilobotSim
    if not torch.cuda.is_available():
        sys.exit('bench_targets needs a GPU: a time taken anywhere else says nothing')
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
            from tests import targets_ref
            cpu = lambda t: t[:1].cpu().numpy()
            return targets_ref.restate(cpu(sim.x), cpu(sim.y), cpu(sim.theta), points.cpu().numpy(), tol)
        except Exception as err:      # noqa: BLE001
            print('no restatement: %s' % err, file=sys.stderr)
            return None

    sim = KilobotSim(E, N, device=dev, allow_sleep=0)
    x, y, th, actions = bench.make_scene(torch, E, N, dev, args.seed, 0, 0)
    sim.x.copy_(x); sim.y.copy_(y); sim.theta.copy_(th)
    sim.forget_contacts()
    for s in range(args.settle):
        sim.step(1, actions=actions[s % len(actions)])
    torch.cuda.synchronize()
    status = int(sim.status.max().item())

    def torch_match(points, index, d_bot, owner, d_slot):
        """Leg (b): both nearest partners by broadcasting, chunk of envs by chunk."""
        tx, ty = points[:, 0] * 25.0, points[:, 1] * 25.0
        chunk = max(1, (args.chunk_mib << 20) // (4 * N * points.shape[0]))
        for at in range(0, E, chunk):
            ex = tx[None, None, :] - sim.x[at:at + chunk, :, None]
            ey = ty[None, None, :] - sim.y[at:at + chunk, :, None]
            d2 = ex * ex + ey * ey
            best, who = d2.min(2)
            index[at:at + chunk] = who
            d_bot[at:at + chunk] = best.sqrt() / 25.0
            best, who = d2.min(1)
            owner[at:at + chunk] = who
            d_slot[at:at + chunk] = best.sqrt() / 25.0

    cov = (torch.empty(E, 48, 64, dtype=torch.int32, device=dev), torch.empty(E, 48, 64, dtype=torch.float32, device=dev),
           torch.empty(E, N, 4, dtype=torch.float32, device=dev), torch.empty(E, 2, dtype=torch.float32, device=dev))
    legs = []
    for K in sizes:
        points = torch.from_numpy(lattice(K)).to(dev)
        index = torch.empty(E, N, dtype=torch.int32, device=dev)
        rel = torch.empty(E, N, 4, dtype=torch.float32, device=dev)
        owner = torch.empty(E, K, dtype=torch.int32, device=dev)
        dist = torch.empty(E, K, dtype=torch.float32, device=dev)
        stats = torch.empty(E, 6, dtype=torch.float32, device=dev)
        t_all, t_rel, t_cov, t_torch = [], [], [], []
        for _ in range(args.repeats):
            t_all.append(timed(lambda: sim.targets(points, args.tol, out=(index, rel, owner, dist, stats)), args.launches))
            t_rel.append(timed(lambda: sim.targets(points, args.tol, owner=False, dist=False, stats=False, out=(index, rel)), args.launches))
            t_cov.append(timed(lambda: sim.coverage(64, 48, out=cov), args.launches))
        sim.targets(points, args.tol, out=(index, rel, owner, dist, stats))
        torch.cuda.synchronize()
        want = restated(sim, points, args.tol)
        same = None if want is None else bool(all(np.array_equal(t[0].cpu().numpy().view(np.uint32), w[0].view(np.uint32))
                                                  for t, w in zip((index, rel, owner, dist, stats), want)))
        assert same is not False, 'env 0 differs from the restatement'
        assert int(index.min()) >= 0 and int(index.max()) < K and int(owner.min()) >= 0 and int(owner.max()) < N
        leg = {'slots': K, 'all_outputs_ms': round(float(np.median(t_all)), 4), 'all_outputs_ms_all': [round(v, 4) for v in t_all],
               'index_rel_ms': round(float(np.median(t_rel)), 4), 'index_rel_ms_all': [round(v, 4) for v in t_rel],
               'kb_sense_coverage_64x48_ms': round(float(np.median(t_cov)), 4), 'kb_sense_coverage_64x48_ms_all': [round(v, 4) for v in t_cov],
               'ratio_to_kb_sense_coverage': round(float(np.median(t_all) / np.median(t_cov)), 2),
               'distance_evaluations_per_call': 2 * E * N * K,
               'evaluations_per_ns': round(2 * E * N * K / (float(np.median(t_all)) * 1e6), 2),
               'mutual_share': round(float(rel[..., 3].mean()), 4), 'filled_slots_share': round(float(stats[:, 4].mean()) / K, 4),
               'env_0_equals_the_restatement': same}
        if not args.no_torch:
            t_index, t_owner = torch.empty(E, N, dtype=torch.int64, device=dev), torch.empty(E, K, dtype=torch.int64, device=dev)
            t_db, t_ds = torch.empty(E, N, device=dev), torch.empty(E, K, device=dev)
            for _ in range(args.repeats):
                t_torch.append(timed(lambda: torch_match(points, t_index, t_db, t_owner, t_ds), args.torch_launches))
            torch.cuda.synchronize()
            leg.update({'torch_ms': round(float(np.median(t_torch)), 3), 'torch_ms_all': [round(v, 3) for v in t_torch],
                        'torch_over_all_outputs': round(float(np.median(t_torch) / np.median(t_all)), 1),
                        'torch_names_the_same_slot': round(float((t_index == index).float().mean()), 6),
                        'torch_names_the_same_owner': round(float((t_owner == owner).float().mean()), 6)})
            del t_index, t_owner, t_db, t_ds
        legs.append(leg)
        del index, rel, owner, dist, stats
        torch.cuda.empty_cache()
    line = {'metric': 'kb_sense_targets_ms', 'envs': E, 'bots': N, 'tol_m': args.tol, 'settle_substeps': args.settle, 'launches_per_timing': args.launches,
            'torch_launches_per_timing': args.torch_launches, 'repeats': args.repeats, 'torch_chunk_mib': args.chunk_mib, 'status': status,
            'timer': 'device events around back-to-back calls, the legs alternately, median of the repeats',
            'library': os.path.basename(nat.LIB_PATH), 'device': torch.cuda.get_device_name(0), 'legs': legs}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
