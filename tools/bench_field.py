#!/usr/bin/env python3
"""Times kb_field_step on the settled cfg3 scene of bench.py (4096 envs x 1024 kilobots), next to the torch sequence it
replaces and to kb_sense_grid with the count plane at the same grid.

usage: tools/bench_field.py [--envs 4096] [--bots 1024] [--grids 64x48,128x96] [--iters 0,1,4,16] [--channels 1,2]
                            [--launches 20] [--repeats 3] [--out FILE]

Per grid, channel count and iteration count: (fused) one kb_field_step with deposit, iterations and sense rows, in place on
its field; (torch) the same update on a field of its own, on the same poses and amounts: the cells of the kilobots, an
index_add_ of the float amounts into the flattened planes (atomic adds: its sums depend on the order), one replicate-padded
5-point stencil per iteration, five gathers per kilobot and the rotation into its frame.  Per grid and channel count also the
deposit alone (iters = 0, no rows) next to (grid) kb_sense_grid with the count plane, which bins the same kilobots into the
same cells and writes one plane per env.  The legs of a shape are timed alternately, `--repeats` times; every time is the mean
over `--launches` back-to-back calls between two device events after a warm-up of the same shape; the median is reported and
all repeats kept beside it.  keep = 0.9 keeps the field bounded over the repeated in-place calls.
Checked outside the timed windows: env 0 of one call from a zero field equals the numpy restatement of the definition
(tests/field_ref.py) bit for bit when the oracle library is there to give its sine and cosine, and the largest difference
between the torch field and the fused one after one call from the same start is reported (torch adds floats).
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KEEP, SPREAD = 0.9, 0.2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--bots', type=int, default=1024)
    ap.add_argument('--grids', default='64x48,128x96')
    ap.add_argument('--iters', default='0,1,4,16')
    ap.add_argument('--channels', default='1,2')
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--torch-launches', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--settle', type=int, default=120, help='substeps before the state is taken')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    import torch.nn.functional as TF
    import bench
    from gym_kilobots_amd import _native as nat
    from gym_kilobots_amd.sim import KilobotSim
    if not torch.cuda.is_available():
        sys.exit('bench_field needs a GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    E, N = args.envs, args.bots
    grids = [tuple(int(v) for v in f.split('x')) for f in args.grids.split(',')]
    iters_list = [int(v) for v in args.iters.split(',')]
    channels = [int(v) for v in args.channels.split(',')]

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
    xmin, xmax, ymin, ymax = (float(v) for v in sim.outline().arena)

    def torch_step(field, amount, iters, rows):
        """The torch leg: deposit, `iters` stencils, gathers and rotation; returns the new field (the stencil is out of place)."""
        C, gh, gw = field.shape[1:]
        icw, ich = gw / (xmax - xmin), gh / (ymax - ymin)
        ix = ((sim.x - xmin) * icw).clamp_(0, gw - 1).long()
        iy = ((sim.y - ymin) * ich).clamp_(0, gh - 1).long()
        flat = iy * gw + ix                                                                       # [E, N]
        at = (torch.arange(E, device=dev)[:, None, None] * C + torch.arange(C, device=dev)[None, None, :]) * (gh * gw) + flat[:, :, None]
        dep = torch.zeros_like(field)
        dep.view(-1).index_add_(0, at.reshape(-1), amount.reshape(-1))
        field = field + dep
        for _ in range(iters):
            p = TF.pad(field, (1, 1, 1, 1), mode='replicate')
            lap = ((p[:, :, 1:-1, :-2] + p[:, :, 1:-1, 2:]) + (p[:, :, :-2, 1:-1] + p[:, :, 2:, 1:-1])) - 4.0 * field
            field = KEEP * (field + SPREAD * lap)
        planes = field.view(E, C, gh * gw)

        def at_cells(jx, jy):
            return planes.gather(2, (jy * gw + jx)[:, None, :].expand(E, C, N)).transpose(1, 2)      # [E, N, C]
        dx = (at_cells((ix + 1).clamp_(max=gw - 1), iy) - at_cells((ix - 1).clamp_(min=0), iy)) * (0.5 * icw * 25.0)
        dy = (at_cells(ix, (iy + 1).clamp_(max=gh - 1)) - at_cells(ix, (iy - 1).clamp_(min=0))) * (0.5 * ich * 25.0)
        c, s = sim.theta.cos()[:, :, None], sim.theta.sin()[:, :, None]
        rows[..., 0], rows[..., 1], rows[..., 2] = at_cells(ix, iy), c * dx + s * dy, c * dy - s * dx
        rows[..., 3] = dep.view(E, C, gh * gw).gather(2, flat[:, None, :].expand(E, C, N)).transpose(1, 2)
        return field

    def restated_equal(gw, gh, C, amount, iters):
        """Whether env 0 of one fused call from a zero field equals the numpy restatement; None where the oracle library cannot be built."""
        field = sim.new_field(gw, gh, C)
        rows = sim.field_step(field, amount, KEEP, SPREAD, iters)
        torch.cuda.synchronize()
        try:
            from tests import field_ref, objects_ref
            cpu = lambda t: t[:1].cpu().numpy()
            G, R = field_ref.restate(objects_ref.tables(sim.outline()), np.zeros((1, C, gh, gw), np.float32), cpu(sim.x), cpu(sim.y), cpu(sim.theta),
                                     cpu(amount), KEEP, SPREAD, iters)
        except Exception as err:      # noqa: BLE001
            print('no restatement: %s' % err, file=sys.stderr)
            return None
        return bool(np.array_equal(cpu(field).view(np.uint32), G.view(np.uint32)) and np.array_equal(cpu(rows).view(np.uint32), R.view(np.uint32)))

    legs = []
    for gw, gh in grids:
        count = torch.empty(E, 1, gh, gw, dtype=torch.float32, device=dev)
        for C in channels:
            amount = torch.rand(E, N, C, device=dev, generator=torch.Generator(dev).manual_seed(args.seed + C))
            field, rows = sim.new_field(gw, gh, C), torch.empty(E, N, C, 4, device=dev)
            tfield, trows = [sim.new_field(gw, gh, C)], torch.empty(E, N, C, 4, device=dev)

            def torch_call(iters):
                tfield[0] = torch_step(tfield[0], amount, iters, trows)
            t_dep, t_grid = [], []
            for _ in range(args.repeats):
                t_dep.append(timed(lambda: sim.field_step(field, amount, KEEP, SPREAD, 0, sense=False), args.launches))
                t_grid.append(timed(lambda: sim.occupancy_grid(gw, gh, ('count',), out=count), args.launches))
            base = {'grid': [gw, gh], 'channels': C, 'deposit_alone_ms': round(float(np.median(t_dep)), 4), 'deposit_alone_ms_all': [round(v, 4) for v in t_dep],
                    'kb_sense_grid_count_ms': round(float(np.median(t_grid)), 4), 'kb_sense_grid_count_ms_all': [round(v, 4) for v in t_grid],
                    'deposit_over_kb_sense_grid': round(float(np.median(t_dep) / np.median(t_grid)), 2)}
            for iters in iters_list:
                same = restated_equal(gw, gh, C, amount, iters)
                assert same is not False, 'env 0 differs from the restatement'
                a, b = sim.new_field(gw, gh, C), sim.new_field(gw, gh, C)
                sim.field_step(a, amount, KEEP, SPREAD, iters, sense=False)
                diff = float((torch_step(b, amount, iters, trows) - a).abs().max())
                del a, b
                field.zero_(); tfield[0].zero_()
                t_fused, t_torch = [], []
                for _ in range(args.repeats):
                    t_fused.append(timed(lambda: sim.field_step(field, amount, KEEP, SPREAD, iters, out=rows), args.launches))
                    t_torch.append(timed(lambda: torch_call(iters), args.torch_launches))
                legs.append(dict(base, iters=iters, fused_ms=round(float(np.median(t_fused)), 4), fused_ms_all=[round(v, 4) for v in t_fused],
                                 torch_ms=round(float(np.median(t_torch)), 3), torch_ms_all=[round(v, 3) for v in t_torch],
                                 torch_over_fused=round(float(np.median(t_torch) / np.median(t_fused)), 2),
                                 max_abs_diff_torch_vs_fused=diff, env_0_equals_the_restatement=same))
            del field, rows, tfield, trows, amount
            torch.cuda.empty_cache()
        del count
    line = {'metric': 'kb_field_step_ms', 'envs': E, 'bots': N, 'keep': KEEP, 'spread': SPREAD, 'settle_substeps': args.settle, 'launches_per_timing': args.launches,
            'torch_launches_per_timing': args.torch_launches, 'repeats': args.repeats, 'status': status,
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
