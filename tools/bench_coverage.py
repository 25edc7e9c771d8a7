#!/usr/bin/env python3
"""Times kb_sense_coverage on the settled cfg3 scene of bench.py (4096 envs x 1024 kilobots), next to kb_render at the same
width x height and to the torch formulation it replaces.

usage: tools/bench_coverage.py [--envs 4096] [--bots 1024] [--grids 64x48,128x96,128x128] [--launches 20] [--repeats 3] [--out FILE]

Per grid: kb_sense_coverage with all four outputs and with d_dist alone; (a) kb_render of the kilobot layer at the same
width x height, the same gather over the cell lists with a fixed radius -- what the missing radius costs; (b) torch on the same
state: broadcast squared distances [envs, cells, kilobots] and min / argmin over the kilobots, in chunks of envs that fit
`--chunk-mib` of memory per temporary (owner and dist only: no cells, no stats).  The kernel legs and kb_render are timed
alternately, `--repeats` times; every time is the mean over `--launches` back-to-back calls between two device events after
a warm-up of the same shape (the torch leg: `--torch-launches`); the median is reported and all repeats kept beside it.
Checked outside the timed windows: env 0 equals the numpy restatement of the definition (tests/coverage_ref.py) bit for bit
when the oracle library is there to give its sine and cosine; the share of cells on which torch names the same owner is
reported (it may round d2 otherwise and breaks ties its own way).
KB_HIP_LIB selects another build of the library (the A/B of KB_COVERAGE_RING_COST).
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
    ap.add_argument('--grids', default='64x48,128x96,128x128')
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
        sys.exit('bench_coverage needs a GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    E, N = args.envs, args.bots
    grids = [tuple(int(v) for v in f.split('x')) for f in args.grids.split(',')]

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

    def restated(sim, gw, gh):
        """env 0 by the numpy restatement, or None where the oracle library cannot be built."""
        try:
            from tests import coverage_ref, objects_ref
            cpu = lambda t: t[:1].cpu().numpy()
            return coverage_ref.restate(objects_ref.tables(sim.outline()), gw, gh, cpu(sim.x), cpu(sim.y), cpu(sim.theta))
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
    xmin, xmax, ymin, ymax = (float(v) for v in sim.outline().arena)

    def torch_fields(gw, gh, owner, dist):
        """Leg (b): the nearest kilobot of every cell centre by broadcasting, chunk of envs by chunk."""
        cx = xmin + (torch.arange(gw, device=dev, dtype=torch.float32) + 0.5) * ((xmax - xmin) / gw)
        cy = ymin + (torch.arange(gh, device=dev, dtype=torch.float32) + 0.5) * ((ymax - ymin) / gh)
        cx, cy = cx.repeat(gh), cy.repeat_interleave(gw)
        chunk = max(1, (args.chunk_mib << 20) // (4 * gw * gh * N))
        for at in range(0, E, chunk):
            ex = sim.x[at:at + chunk, None, :] - cx[None, :, None]
            ey = sim.y[at:at + chunk, None, :] - cy[None, :, None]
            d2, who = (ex * ex + ey * ey).min(-1)
            owner[at:at + chunk] = who.view(-1, gh, gw)
            dist[at:at + chunk] = (d2.sqrt() / 25.0).view(-1, gh, gw)

    legs = []
    for gw, gh in grids:
        owner = torch.empty(E, gh, gw, dtype=torch.int32, device=dev)
        dist = torch.empty(E, gh, gw, dtype=torch.float32, device=dev)
        cells = torch.empty(E, N, 4, dtype=torch.float32, device=dev)
        stats = torch.empty(E, 2, dtype=torch.float32, device=dev)
        rgb = torch.empty(E, gh, gw, 3, dtype=torch.uint8, device=dev)
        t_all, t_dist, t_render, t_torch = [], [], [], []
        for _ in range(args.repeats):
            t_all.append(timed(lambda: sim.coverage(gw, gh, out=(owner, dist, cells, stats)), args.launches))
            t_dist.append(timed(lambda: sim.coverage(gw, gh, owner=False, cells=False, stats=False, out=dist), args.launches))
            t_render.append(timed(lambda: sim.render(gw, gh, layers=('bots',), out=rgb), args.launches))
        sim.coverage(gw, gh, out=(owner, dist, cells, stats))
        torch.cuda.synchronize()
        want = restated(sim, gw, gh)
        same = None if want is None else bool(all(np.array_equal(t[0].cpu().numpy().view(np.uint32), w[0].view(np.uint32))
                                                  for t, w in zip((owner, dist, cells, stats), want)))
        assert same is not False, 'env 0 differs from the restatement'
        assert int(owner.min()) >= 0 and int(owner.max()) < N
        leg = {'grid': [gw, gh], 'all_outputs_ms': round(float(np.median(t_all)), 4), 'all_outputs_ms_all': [round(v, 4) for v in t_all],
               'dist_alone_ms': round(float(np.median(t_dist)), 4), 'dist_alone_ms_all': [round(v, 4) for v in t_dist],
               'kb_render_ms': round(float(np.median(t_render)), 4), 'kb_render_ms_all': [round(v, 4) for v in t_render],
               'ratio_to_kb_render': round(float(np.median(t_all) / np.median(t_render)), 2),
               'mean_cost_m2_per_cell': round(float(stats[:, 0].mean()) / (gw * gh), 6), 'worst_covered_m': round(float(stats[:, 1].max()), 4),
               'kilobots_without_a_cell': int((cells[..., 2] == 0).sum()), 'env_0_equals_the_restatement': same}
        if not args.no_torch:
            t_owner, t_d = torch.empty_like(owner), torch.empty_like(dist)
            for _ in range(args.repeats):
                t_torch.append(timed(lambda: torch_fields(gw, gh, t_owner, t_d), args.torch_launches))
            torch.cuda.synchronize()
            leg.update({'torch_ms': round(float(np.median(t_torch)), 3), 'torch_ms_all': [round(v, 3) for v in t_torch],
                        'torch_over_all_outputs': round(float(np.median(t_torch) / np.median(t_all)), 1),
                        'torch_over_dist_alone': round(float(np.median(t_torch) / np.median(t_dist)), 1),
                        'torch_names_the_same_owner': round(float((t_owner == owner).float().mean()), 6)})
            del t_owner, t_d
        legs.append(leg)
        del owner, dist, cells, stats, rgb
        torch.cuda.empty_cache()
    line = {'metric': 'kb_sense_coverage_ms', 'envs': E, 'bots': N, 'settle_substeps': args.settle, 'launches_per_timing': args.launches,
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
