#!/usr/bin/env python3
"""Times kb_sense_reduce on the settled cfg3 scene of bench.py (4096 envs x 1024 kilobots) next to three baselines.

usage: tools/bench_reduce.py [--envs 4096] [--bots 1024] [--launches 50] [--repeats 3] [--out FILE]

Legs: (R, op, channels) = (0.07, sum, 4), (0.07, sum, 8), (0.15, min, 1), (0.15, sum, 4); messages uniform in [-1, 1],
scale 65536.  Baselines on the same poses and radius:
  kb_sense            the count alone: the same walk over half the stencil, 4 B per kilobot -- a lower bound;
  kb_sense_histogram  (R, 4, 8): the same full walk with a heavier accumulator and 128 B out per kilobot;
  torch               a chunked restatement a user of poses() would write: cdist -> range mask -> bmm with the messages
                      (sum) or a masked amin (min).
Every time is the mean over `--launches` back-to-back launches between two device events after a warm-up of the same
shape; the legs are interleaved and repeated `--repeats` times, the median is reported and the spread kept beside it.
Checked on every leg, outside the timed windows: the kernel's counts equal kb_sense's; with the library's own predicate
evaluated in torch, the sum is within count * 0.5 / scale + |exact| * 2^-23 of the float64 sum at EVERY kilobot; and the
torch restatement (float64 for this check) agrees within the same bound -- the min exactly -- at every kilobot but those
with a pair on the rim, which cdist rounds differently: those pairs are counted into the line.
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = [(0.07, 'sum', 4), (0.07, 'sum', 8), (0.15, 'min', 1), (0.15, 'sum', 4)]
SCALE = 65536.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--bots', type=int, default=1024)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--settle', type=int, default=120, help='substeps before the poses are taken')
    ap.add_argument('--chunk', type=int, default=32, help='envs per torch pass (32 x 1024 x 1024 floats = 128 MiB per temporary)')
    ap.add_argument('--torch-passes', type=int, default=1)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    import bench
    from gym_kilobots_amd.sim import KilobotSim
    if not torch.cuda.is_available():
        sys.exit('bench_reduce needs a GPU: a time taken anywhere else says nothing')
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

    xy = sim.poses()[..., :2].contiguous()
    eye = torch.eye(N, dtype=torch.bool, device=dev)
    inf = torch.tensor(float('inf'), device=dev)

    def torch_reduce(R, op, values, out):
        for a in range(0, E, args.chunk):
            p, v = xy[a:a + args.chunk], values[a:a + args.chunk]
            inr = (torch.cdist(p, p) <= R) & ~eye
            if op == 'sum':
                torch.bmm(inr.float(), v, out=out[a:a + args.chunk])
            else:
                out[a:a + args.chunk] = torch.where(inr[..., None], v[:, None], inf).amin(2)
        return out

    def compare(R, op, values, got, cnt):
        """(kilobots whose result misses the bound against the library's predicate in float64, pairs on the rim, kilobots
        with such a pair, kilobots without one where the torch restatement (float64) disagrees)."""
        Rw = np.float32(R) * np.float32(25)
        R2 = float(Rw * Rw)
        miss = rim = rim_bots = differ = 0
        for a in range(0, E, args.chunk):
            sl = slice(a, a + args.chunk)
            ex = sim.x[sl, None, :] - sim.x[sl, :, None]
            ey = sim.y[sl, None, :] - sim.y[sl, :, None]
            d2 = ex * ex
            d2 += ey * ey                       # (two products, one sum, each rounded on its own: the library's predicate)
            exact = ~(d2 > R2) & ~eye
            del ex, ey, d2
            loose = (torch.cdist(xy[sl], xy[sl]) <= R) & ~eye
            off = exact != loose
            rim += int(off.sum().item())
            clean = ~off.any(2)
            rim_bots += int((~clean).sum().item())
            v, g = values[sl].double(), got[sl].double()
            assert torch.equal(exact.sum(2).int(), cnt[sl])
            if op == 'sum':
                for mask, rows in ((exact, None), (loose, clean)):
                    want = torch.bmm(mask.double(), v)
                    bad = (g - want).abs() > mask.sum(2, keepdim=True) * (0.5 / SCALE) + want.abs() * 2.0 ** -23
                    if rows is None:
                        miss += int(bad.any(2).sum().item())
                    else:
                        differ += int((bad.any(2) & rows).sum().item())
            else:
                for mask, rows in ((exact, None), (loose, clean)):
                    bad = g != torch.where(mask[..., None], v[:, None], inf.double()).amin(2)
                    if rows is None:
                        miss += int(bad.any(2).sum().item())
                    else:
                        differ += int((bad.any(2) & rows).sum().item())
        return miss, rim, rim_bots, differ

    legs = []
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed + 1)
    for R, op, C in LEGS:
        values = torch.rand(E, N, C, device=dev, generator=gen) * 2.0 - 1.0
        out = torch.empty(E, N, C, dtype=torch.float32, device=dev)
        cnt = torch.empty(E, N, dtype=torch.int32, device=dev)
        rcnt = torch.empty(E, N, dtype=torch.int32, device=dev)
        hist = torch.empty(E, N, 4, 8, dtype=torch.float32, device=dev)
        t_out = torch.empty(E, N, C, dtype=torch.float32, device=dev)
        t_r, t_se, t_h, t_to = [], [], [], []
        for _ in range(args.repeats):
            t_r.append(timed(lambda: sim.neighbor_reduce(values, R, op=op, scale=SCALE, out=out), args.launches))
            t_se.append(timed(lambda: sim.sense(R, out=cnt), args.launches))
            t_h.append(timed(lambda: sim.neighbor_histogram(R, 4, 8, out=hist), args.launches))
            t_to.append(timed(lambda: torch_reduce(R, op, values, t_out), args.torch_passes))
        sim.neighbor_reduce(values, R, op=op, scale=SCALE, out=(out, rcnt), count=True)
        torch.cuda.synchronize()
        assert torch.equal(rcnt, cnt)
        del hist, t_out
        miss, rim, rim_bots, differ = compare(R, op, values, out, cnt)
        assert miss == 0, 'kb_sense_reduce misses its bound at %d kilobots' % miss
        assert differ == 0, 'the torch restatement disagrees at %d kilobots without a pair on the rim' % differ
        ms, ms_sense, ms_hist, ms_torch = (float(np.median(v)) for v in (t_r, t_se, t_h, t_to))
        assert ms < ms_torch, 'kb_sense_reduce (%.3f ms) is not faster than the torch restatement (%.3f ms)' % (ms, ms_torch)
        out_bytes = E * N * C * 4
        gbs = out_bytes / (ms * 1e-3) / 1e9
        legs.append({'radius_m': R, 'op': op, 'n_channels': C, 'scale': SCALE, 'ms': round(ms, 4), 'ms_all': [round(v, 4) for v in t_r],
                     'kb_sense_ms': round(ms_sense, 4), 'kb_sense_ms_all': [round(v, 4) for v in t_se], 'ratio_to_kb_sense': round(ms / ms_sense, 3),
                     'kb_sense_histogram_4x8_ms': round(ms_hist, 4), 'kb_sense_histogram_ms_all': [round(v, 4) for v in t_h],
                     'ratio_to_kb_sense_histogram': round(ms / ms_hist, 3),
                     'torch_ms': round(ms_torch, 3), 'torch_ms_all': [round(v, 3) for v in t_to], 'speedup_over_torch': round(ms_torch / ms, 1),
                     'output_bytes': out_bytes, 'output_gb_per_s': round(gbs, 1), 'hbm_roof_frac': round(gbs / bench.HBM_PEAK_GBS, 4),
                     'mean_in_range': round(float(cnt.float().mean().item()), 2), 'max_in_range': int(cnt.max().item()),
                     'kilobots_missing_the_bound': miss, 'pairs_on_the_rim_torch_rounds_differently': rim,
                     'kilobots_with_a_rim_pair': rim_bots, 'other_kilobots_where_torch_differs': differ})
        del values, out
    line = {'metric': 'kb_sense_reduce_ms', 'envs': E, 'bots': N, 'scene': 'cfg3 lattice after %d substeps' % args.settle,
            'launches_per_timing': args.launches, 'repeats': args.repeats, 'timer': 'device events around back-to-back launches, median of the repeats',
            'torch_baseline': 'torch.cdist -> range mask -> bmm (sum) or masked amin (min) in chunks of %d envs, %d passes per timing' % (args.chunk, args.torch_passes),
            'hbm_peak_gb_per_s': bench.HBM_PEAK_GBS, 'device': torch.cuda.get_device_name(0), 'legs': legs}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
