#!/usr/bin/env python3
"""Times kb_sense_edges on the settled cfg3 scene of bench.py (4096 envs x 1024 kilobots), next to kb_sense_neighbors.

usage: tools/bench_edges.py [--envs 4096] [--bots 1024] [--radii 0.07,0.1] [--launches 20] [--repeats 10] [--out FILE]

Radii of 0.07 and 0.1 m.  The edge list is written into preallocated outputs (src, dst, rel) from offsets computed beforehand,
so the timed call is the one launch of the library.  The yardstick is kb_sense_neighbors(R, 16) on the same state at the same
radius: it builds the same cell lists, walks the same stencil and writes 16 slots of 20 bytes per kilobot, about what the edge
list of the settled lattice at 0.07 m writes.  The two are timed alternately in the same process, `--repeats` times; every time
is the mean over `--launches` back-to-back launches between two device events after a warm-up of the same shape; the median is
reported and all repeats kept beside it.  What a caller pays to get the offsets -- kb_sense and torch.cumsum into int64 -- is
timed the same way as a line of its own.
Reported per radius: ms, nnz, the bytes the call writes (24 per edge: src, dst, rel; plus 4 per kilobot where the counts are
written, which the timed call does not ask for), the GB/s of those bytes, and the ratio to the yardstick.
Checked outside the timed windows: env 0 equals the numpy restatement of the definition (tests/edges_ref.py) bit for bit when
the oracle library is there to give its sine and cosine.
KB_HIP_LIB selects another build of the library (the A/B of the emission).
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
        sys.exit('bench_edges needs a GPU: a time taken anywhere else says nothing')
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

    def env0_equals_the_restatement(sim, R, ed):
        """env 0 against the numpy restatement, or None where the oracle library cannot be built."""
        try:
            from tests import edges_ref
            cpu = lambda t: t[:1].cpu().numpy()
            src, dst, rel, count, offsets = edges_ref.restate(cpu(sim.x), cpu(sim.y), cpu(sim.theta), R)
        except Exception as err:      # noqa: BLE001
            print('no restatement: %s' % err, file=sys.stderr)
            return None
        n = len(src)
        return bool(int(ed.offsets[N]) == n and np.array_equal(ed.src[:n].cpu().numpy(), src) and np.array_equal(ed.dst[:n].cpu().numpy(), dst)
                    and np.array_equal(ed.rel[:n].cpu().numpy().view(np.uint32), rel.view(np.uint32))
                    and np.array_equal(ed.count[0].cpu().numpy().view(np.uint32), count[0]))

    sim = KilobotSim(E, N, device=dev, allow_sleep=0)
    x, y, th, actions = bench.make_scene(torch, E, N, dev, args.seed, 0, 0)
    sim.x.copy_(x); sim.y.copy_(y); sim.theta.copy_(th)
    sim.forget_contacts()
    for s in range(args.settle):
        sim.step(1, actions=actions[s % len(actions)])
    torch.cuda.synchronize()
    status = int(sim.status.max().item())
    nbr = sim.neighbors(radii[0], 16)
    legs = []
    for R in radii:
        ed = sim.edges(R)                       # sizes the outputs; they are reused below
        nnz = ed.nnz
        count = torch.empty(E, N, dtype=torch.int32, device=dev)
        offsets = torch.zeros(E * N + 1, dtype=torch.int64, device=dev)

        def setup():
            sim.sense(R, out=count)
            torch.cumsum(count.view(-1), 0, dtype=torch.int64, out=offsets[1:])
        t_e, t_n, t_s = [], [], []
        for _ in range(args.repeats):
            t_e.append(timed(lambda: sim._sense_edges(R, ed.offsets, nnz, ed.src, ed.dst, ed.rel, None), args.launches))
            t_n.append(timed(lambda: sim.neighbors(R, 16, out=nbr), args.launches))
            t_s.append(timed(setup, args.launches))
        torch.cuda.synchronize()
        assert torch.equal(offsets, ed.offsets)
        same = env0_equals_the_restatement(sim, R, ed)
        assert same is not False, 'env 0 differs from the restatement'
        ms, ms_n, ms_s = float(np.median(t_e)), float(np.median(t_n)), float(np.median(t_s))
        written = 24 * nnz
        cnt = ed.count.view(-1).long()
        legs.append({'radius_m': R, 'nnz': nnz, 'edges_per_kilobot': round(nnz / (E * N), 3), 'longest_row': int(cnt.max().item()),
                     'rows_above_16': int((cnt > 16).sum().item()),
                     'ms': round(ms, 4), 'ms_all': [round(v, 4) for v in t_e], 'bytes_written': written, 'bytes_of_the_counts_not_asked_for': 4 * E * N,
                     'GBps_written': round(written / (ms * 1e-3) / 1e9, 1), 'ns_per_edge': round(ms * 1e6 / max(nnz, 1), 4),
                     'kb_sense_neighbors_16_ms': round(ms_n, 4), 'kb_sense_neighbors_16_ms_all': [round(v, 4) for v in t_n],
                     'kb_sense_neighbors_16_bytes_written': 16 * 20 * E * N + 4 * E * N,
                     'ratio_to_kb_sense_neighbors': round(ms / ms_n, 2),
                     'kb_sense_plus_cumsum_ms': round(ms_s, 4), 'kb_sense_plus_cumsum_ms_all': [round(v, 4) for v in t_s],
                     'env_0_equals_the_restatement': same})
        del ed, count, offsets
        torch.cuda.empty_cache()
    line = {'metric': 'kb_sense_edges_ms', 'envs': E, 'bots': N, 'scene': 'cfg3: settled lattice', 'status': status, 'settle_substeps': args.settle,
            'launches_per_timing': args.launches, 'repeats': args.repeats,
            'timer': 'device events around back-to-back launches; kb_sense_edges, kb_sense_neighbors and kb_sense + cumsum alternately, median of the repeats',
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
