#!/usr/bin/env python3
"""Times kb_sense_paths on the settled cfg4 scene of bench.py (4096 envs x 1024 kilobots, four discs), next to three
yardsticks on the same state.

usage: tools/bench_paths.py [--envs 4096] [--bots 1024] [--grids 64x48,128x96,128x128] [--legs empty,discs,serpentine]
                            [--launches 10] [--repeats 3] [--out FILE]

Legs, per grid: (empty) one source in a corner of an empty table; (discs) the same source with the four discs blocking at the
clearance of a kilobot radius; (serpentine) a d_blocked of alternating walls with a gap at one end, one corridor through
every other row: the worst case for the sweep count.  Each leg is timed with d_dist alone and with all four outputs.
Yardsticks: (torch) the loop the kernel replaces, an int32 min-plus stencil over [E, gh, gw] with the same moves and the same
corner rule, iterated to the fixed point with the convergence check (one host sync) every eight sweeps, on the blocked plane
the kernel derived (what making that plane costs is the grid yardstick); (field)
kb_field_step without deposit and rows with as many iterations as that loop needed sweeps, in calls of at most
KB_FIELD_MAX_ITERS: the same plane-in-LDS stencil, so its time over the sweeps is what a Jacobi sweep of such a plane costs;
(grid) kb_sense_grid with the object planes: the cost of the blocked-plane pass.
The sweep count reported per leg is that of the torch loop, a Jacobi iteration: the longest shortest path in moves, plus
the sweep that changes nothing.  The kernel relaxes in place and needs no more sweeps than that; it does not report its own.
The legs of a shape are timed alternately, `--repeats` times; every kernel time is the mean over `--launches` back-to-back
calls between two device events after a warm-up of the same shape; the torch loop is timed by the wall clock
around a synchronised run (it syncs by itself) after a warm-up of eight sweeps, `--torch-repeats` times (default once: its
worst leg runs for a minute).  The median is reported and all repeats kept beside it.
Checked outside the timed windows: the torch loop's distances equal the kernel's in every cell of every env.
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KILOBOT_RADIUS = 0.0165
DIRS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))
BIG = 1 << 30


def serpentine(gw, gh):
    blk = np.zeros((gh, gw), dtype=np.uint8)
    for n, iy in enumerate(range(1, gh, 2)):
        blk[iy, :] = 1
        blk[iy, gw - 1 if n % 2 == 0 else 0] = 0
    return blk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--bots', type=int, default=1024)
    ap.add_argument('--grids', default='64x48,128x96,128x128')
    ap.add_argument('--legs', default='empty,discs,serpentine')
    ap.add_argument('--launches', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--torch-repeats', type=int, default=1)
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
        sys.exit('bench_paths needs a GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    E, N, M = args.envs, args.bots, 4
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

    sim = KilobotSim(E, N, device=dev, num_objects=M, allow_sleep=0)
    x, y, th, actions = bench.make_scene(torch, E, N, dev, args.seed, 0, M)
    sim.x.copy_(x); sim.y.copy_(y); sim.theta.copy_(th)
    sim.set_objects_m(np.tile(bench.CFG4_OBJECTS[None, :M], (E, 1, 1)))
    sim.forget_contacts()
    for s in range(args.settle):
        sim.step(1, actions=actions[s % len(actions)])
    torch.cuda.synchronize()
    status = int(sim.status.max().item())

    def torch_loop(source, blocked, q, most=None):
        """The int32 min-plus stencil to the fixed point (or for `most` sweeps: the warm-up); returns (D with BIG where there
        is no path, sweeps)."""
        qx, qy, qd = q
        w = [qd if k & 1 else qy if k & 2 else qx for k in range(8)]
        free = ~blocked
        fpad = TF.pad(free, (1, 1, 1, 1), value=False)
        gh, gw = source.shape[1:]

        def shifted(p, dx, dy):
            return p[:, 1 + dy:1 + dy + gh, 1 + dx:1 + dx + gw]
        ok = []
        for k, (dx, dy) in enumerate(DIRS):
            m = free & shifted(fpad, dx, dy)
            if k & 1:
                m = m & shifted(fpad, dx, 0) & shifted(fpad, 0, dy)
            ok.append(m)
        big = torch.full((), BIG, dtype=torch.int32, device=dev)
        D = torch.where(source & free, torch.zeros((), dtype=torch.int32, device=dev), big).expand(E, gh, gw).contiguous()
        sweeps = 0
        while True:
            before = D
            for _ in range(8):
                p = TF.pad(D, (1, 1, 1, 1), value=BIG)
                new = D
                for k, (dx, dy) in enumerate(DIRS):
                    new = torch.minimum(new, torch.where(ok[k], shifted(p, dx, dy) + w[k], big))     # (BIG + w stays below 2^31)
                D = torch.minimum(new, big)
                sweeps += 1
            if torch.equal(D, before) or (most is not None and sweeps >= most):         # the host sync
                return D, sweeps

    legs = []
    for gw, gh in grids:
        q = sim.path_costs(gw, gh)
        source = torch.zeros(E, gh, gw, dtype=torch.uint8, device=dev)
        source[:, 0, 0] = 1
        walls = torch.from_numpy(np.tile(serpentine(gw, gh), (E, 1, 1))).to(dev)
        planes = torch.empty(E, M, gh, gw, dtype=torch.float32, device=dev)
        field = sim.new_field(gw, gh, 1)
        dist = torch.empty(E, gh, gw, dtype=torch.float32, device=dev)
        outs = (dist, torch.empty(E, gh, gw, dtype=torch.int8, device=dev), torch.empty(E, N, 4, dtype=torch.float32, device=dev),
                torch.empty(E, 4, dtype=torch.float32, device=dev))
        for leg in args.legs.split(','):
            kw = dict(empty=dict(objects=0), discs=dict(objects='all', clearance_m=KILOBOT_RADIUS), serpentine=dict(objects=0, blocked=walls))[leg]
            # the blocked plane the kernel derives, for the torch loop: blocked <=> d_next == -3
            step = sim.paths(gw, gh, source, dist=False, bots=False, stats=False, **kw).step
            blocked = step == -3
            torch_loop(source.bool(), blocked, q, most=8)       # warm-up of this shape
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            D, sweeps = torch_loop(source.bool(), blocked, q)
            torch.cuda.synchronize()
            t_torch = [(time.perf_counter() - t0) * 1e3]
            sim.paths(gw, gh, source, step=False, bots=False, stats=False, out=dist, **kw)
            Df = D.float()      # (tensor divisors: a division by a Python number may become a multiplication by its reciprocal)
            want = torch.where(D < BIG, (Df / torch.full_like(Df, 1024.0)) / torch.full_like(Df, 25.0), torch.full_like(Df, float('inf')))
            differ = int((want.view(torch.int32) != dist.view(torch.int32)).sum())
            same = differ == 0
            if not same:
                print('the torch loop and the kernel differ in %d cells (%s, %d x %d)' % (differ, leg, gw, gh), file=sys.stderr, flush=True)
            del Df, want
            calls = [min(nat.FIELD_MAX_ITERS, sweeps - at) for at in range(0, sweeps, nat.FIELD_MAX_ITERS)]

            def field_sweeps():
                for n in calls:
                    sim.field_step(field, None, 1.0, 0.2, n, sense=False)
            t_dist, t_all, t_field, t_grid = [], [], [], []
            for r in range(args.repeats):
                t_dist.append(timed(lambda: sim.paths(gw, gh, source, step=False, bots=False, stats=False, out=dist, **kw), args.launches))
                t_all.append(timed(lambda: sim.paths(gw, gh, source, out=outs, **kw), args.launches))
                t_field.append(timed(field_sweeps, 1))
                t_grid.append(timed(lambda: sim.occupancy_grid(gw, gh, ('objects',), out=planes), args.launches))
                if r + 1 < args.torch_repeats:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    torch_loop(source.bool(), blocked, q)
                    torch.cuda.synchronize()
                    t_torch.append((time.perf_counter() - t0) * 1e3)
            med = lambda v: float(np.median(v))
            legs.append({'grid': [gw, gh], 'leg': leg, 'step_costs': list(q), 'jacobi_sweeps': sweeps, 'blocked_cells_env0': int(blocked[0].sum()),
                         'reached_cells_env0': int((D[0] < BIG).sum()), 'dist_ms': round(med(t_dist), 4), 'dist_ms_all': [round(v, 4) for v in t_dist],
                         'all_outputs_ms': round(med(t_all), 4), 'all_outputs_ms_all': [round(v, 4) for v in t_all],
                         'torch_loop_ms': round(med(t_torch), 2), 'torch_loop_ms_all': [round(v, 2) for v in t_torch],
                         'torch_over_dist': round(med(t_torch) / med(t_dist), 2),
                         'kb_field_step_same_sweeps_ms': round(med(t_field), 4), 'kb_field_step_same_sweeps_ms_all': [round(v, 4) for v in t_field],
                         'kb_field_step_us_per_sweep': round(1e3 * med(t_field) / sweeps, 3), 'dist_us_per_jacobi_sweep': round(1e3 * med(t_dist) / sweeps, 3),
                         'kb_sense_grid_objects_ms': round(med(t_grid), 4), 'kb_sense_grid_objects_ms_all': [round(v, 4) for v in t_grid],
                         'torch_equals_kernel': same, 'cells_that_differ': differ})
            print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
        del source, walls, planes, field, dist, outs
        torch.cuda.empty_cache()
    line = {'metric': 'kb_sense_paths_ms', 'envs': E, 'bots': N, 'objects': M, 'clearance_m': KILOBOT_RADIUS, 'settle_substeps': args.settle,
            'launches_per_timing': args.launches, 'repeats': args.repeats, 'torch_repeats': args.torch_repeats, 'status': status,
            'timer': 'device events around back-to-back calls, the legs alternately, median of the repeats; the torch loop by the wall clock around a synchronised run',
            'sweeps': 'of the torch loop (Jacobi, checked every eight); the kernel relaxes in place and does not report its own',
            'library': os.path.basename(nat.LIB_PATH), 'device': torch.cuda.get_device_name(0), 'legs': legs}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
