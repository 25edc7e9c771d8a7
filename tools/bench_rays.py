#!/usr/bin/env python3
"""Times kb_sense_rays on the settled cfg3 scene of bench.py (4096 envs x 1024 kilobots) and on its cfg4 variant with four
pushable discs, next to kb_sense_neighbors.

usage: tools/bench_rays.py [--envs 4096] [--bots 1024] [--radii 0.07,0.1] [--rays 8,16,32] [--launches 20] [--repeats 10] [--out FILE]

Radii of 0.07 and 0.1 m, 8, 16 and 32 rays, every target the scene has (kilobots and walls; with the discs, those too).  The
yardstick is kb_sense_neighbors(R, 16) on the same state at the same radius: it builds the same cell lists and walks the same
kind of stencil (kb_sense_rays at the reach of R + r_bot), and keeps 16 keys per kilobot where the scan keeps one per ray.  The
two are timed alternately in the same process, `--repeats` times; every time is the mean over `--launches` back-to-back
launches between two device events after a warm-up of the same shape (10 x 20 = 200 calls each per leg); the median is
reported and all repeats kept beside it.
Checked outside the timed windows: the scan of env 0 equals the numpy restatement of the definition (tests/rays_ref.py) bit
for bit when the oracle library is there to give its sine and cosine, and the rays hit kilobots, walls and nothing.
KB_HIP_LIB selects another build of the library (the A/B of the rays per pass).
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
    ap.add_argument('--radii', default='0.07,0.1')
    ap.add_argument('--rays', default='8,16,32')
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--settle', type=int, default=120, help='substeps before the state is taken')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    import bench
    from gym_kilobots_amd import _native as nat
    from gym_kilobots_amd.sim import KilobotSim
    if not torch.cuda.is_available():
        sys.exit('bench_rays needs a GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    E, N = args.envs, args.bots
    radii = [float(v) for v in args.radii.split(',')]
    counts = [int(v) for v in args.rays.split(',')]

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

    def restated(sim, R, K, targets):
        """env 0 by the numpy restatement, or None where the oracle library cannot be built."""
        try:
            from tests import objects_ref, rays_ref
            cpu = lambda t: t[:1].cpu().numpy()
            obj = (cpu(sim.ox), cpu(sim.oy), cpu(sim.otheta)) if sim.num_objects else (None, None, None)
            return rays_ref.restate(objects_ref.tables(sim.outline()), cpu(sim.x), cpu(sim.y), cpu(sim.theta), *obj, R, sim.cfg.bot_radius, K, targets)
        except Exception as err:      # noqa: BLE001
            print('no restatement: %s' % err, file=sys.stderr)
            return None

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
        targets = nat.RAY_BOTS | nat.RAY_WALLS | (nat.RAY_OBJECTS if M else 0)
        nbr = sim.neighbors(radii[0], 16)
        legs = []
        for R in radii:
            for K in counts:
                out = (torch.empty(E, N, K, dtype=torch.float32, device=dev), torch.empty(E, N, K, dtype=torch.int32, device=dev))
                t_k, t_n = [], []
                for _ in range(args.repeats):
                    t_k.append(timed(lambda: sim.rays(R, K, targets, out=out), args.launches))
                    t_n.append(timed(lambda: sim.neighbors(R, 16, out=nbr), args.launches))
                sim.rays(R, K, targets, out=out)
                torch.cuda.synchronize()
                hit = out[1]
                kinds = {'kilobot': float(((hit >= 0) & (hit < N)).float().mean().item()), 'wall': float(((hit >= N) & (hit < N + 4)).float().mean().item()),
                         'object': float((hit >= N + 4).float().mean().item()), 'nothing': float((hit < 0).float().mean().item())}
                assert kinds['kilobot'] > 0 and kinds['nothing'] > 0, kinds
                want = restated(sim, R, K, targets)
                same = None if want is None else bool(np.array_equal(out[0][:1].cpu().numpy().view(np.uint32), want[0].view(np.uint32))
                                                      and np.array_equal(out[1][:1].cpu().numpy(), want[1]))
                assert same is not False, 'env 0 differs from the restatement'
                ms, ms_n = float(np.median(t_k)), float(np.median(t_n))
                legs.append({'radius_m': R, 'rays': K, 'ms': round(ms, 4), 'ms_all': [round(v, 4) for v in t_k],
                             'kb_sense_neighbors_16_ms': round(ms_n, 4), 'kb_sense_neighbors_16_ms_all': [round(v, 4) for v in t_n],
                             'ratio_to_kb_sense_neighbors': round(ms / ms_n, 2), 'ns_per_ray': round(ms * 1e6 / (E * N * K), 4),
                             'share_of_rays_on': {k: round(v, 4) for k, v in kinds.items()}, 'env_0_equals_the_restatement': same})
                del out
                torch.cuda.empty_cache()
        scenes.append({'scene': name, 'objects': M, 'targets': targets, 'status': status, 'legs': legs})
        sim.close()
        del sim, nbr
        torch.cuda.empty_cache()
    line = {'metric': 'kb_sense_rays_ms', 'envs': E, 'bots': N, 'settle_substeps': args.settle, 'launches_per_timing': args.launches, 'repeats': args.repeats,
            'timer': 'device events around back-to-back launches, kb_sense_rays and kb_sense_neighbors alternately, median of the repeats',
            'library': os.path.basename(nat.LIB_PATH), 'device': torch.cuda.get_device_name(0), 'scenes': scenes}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
