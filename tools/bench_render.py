#!/usr/bin/env python3
"""Times kb_render on the settled cfg3 scene of bench.py (4096 envs x 1024 kilobots) and on its cfg4 variant with four
pushable discs and a circular light, next to kb_get_poses.

usage: tools/bench_render.py [--envs 4096] [--bots 1024] [--frames 64x48,128x96,256x192] [--launches 20] [--repeats 3] [--out FILE]

Frames of 64 x 48, 128 x 96 and 256 x 192, all three layers (on cfg3 only the kilobots draw anything).  The yardstick is
kb_get_poses on the same state, the lightest launch that reads the same poses: 12 B in and 12 B out per kilobot; kb_render
reads 12 B per kilobot once per band of rows and writes 3 width height B per env.  The two are timed alternately in the same
call, `--repeats` times; every time is the mean over `--launches` back-to-back launches between two device events after a
warm-up of the same shape; the median is reported and all repeats kept beside it.  Reported per frame: ms per call, the
bytes written per call, and the ratio to kb_get_poses scaled by the bytes written (ms per byte of kb_render over ms per
byte of kb_get_poses: how much dearer a rendered byte is than a copied one).
Checked outside the timed windows: the frame of env 0 equals the numpy restatement of the definition (tests/render_ref.py)
byte for byte when the oracle library is there to give its sine and cosine, and every frame has kilobot pixels.
KB_HIP_LIB selects another build of the library (the A/B of where the sine and cosine are computed); with
--envs 1 --bots 16 --frames 1200x900 the tool times the reference's screen.
Prints one JSON line (and writes it to --out)."""
import argparse
import ctypes as C
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
    ap.add_argument('--frames', default='64x48,128x96,256x192')
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--settle', type=int, default=120, help='substeps before the state is taken')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    import bench
    from gym_kilobots_amd import _native as nat
    from gym_kilobots_amd.sim import KilobotSim
    if not torch.cuda.is_available():
        sys.exit('bench_render needs a GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    E, N = args.envs, args.bots
    frames = [tuple(int(v) for v in f.split('x')) for f in args.frames.split(',')]

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

    def restated(sim, width, height):
        """env 0 by the numpy restatement, or None where the oracle library cannot be built."""
        try:
            from tests import objects_ref, render_ref
            tab = objects_ref.tables(sim.outline())
            cpu = lambda t: t[:1].cpu().numpy()
            kw = dict(ox=cpu(sim.ox), oy=cpu(sim.oy), oth=cpu(sim.otheta)) if sim.num_objects else {}
            if sim.light_type == nat.LIGHT_CIRCULAR:
                kw['lights'] = ([sim.cfg.light_radius], cpu(sim.light_x).reshape(1, 1), cpu(sim.light_y).reshape(1, 1))
            return render_ref.restate(tab, width, height, render_ref.ALL, sim.cfg.bot_radius, cpu(sim.x), cpu(sim.y), cpu(sim.theta), **kw)[0]
        except Exception as err:      # noqa: BLE001
            print('no restatement: %s' % err, file=sys.stderr)
            return None

    scenes = []
    for name, M in (('cfg3: settled lattice', 0), ('cfg4: cfg3 + four discs + a circular light', 4)):
        sim = KilobotSim(E, N, device=dev, num_objects=M, allow_sleep=0, light_type=nat.LIGHT_CIRCULAR if M else nat.LIGHT_NONE)
        x, y, th, actions = bench.make_scene(torch, E, N, dev, args.seed, 0, M)
        sim.x.copy_(x); sim.y.copy_(y); sim.theta.copy_(th)
        sim.forget_contacts()
        if M:
            sim.set_objects_m(np.tile(bench.CFG4_OBJECTS[None, :M], (E, 1, 1)))
            sim.light_x.fill_(0.1); sim.light_y.fill_(-0.05)
        for s in range(args.settle):
            sim.step(1, actions=actions[s % len(actions)])
        torch.cuda.synchronize()
        status = int(sim.status.max().item())
        poses = torch.empty(E, N, 3, dtype=torch.float32, device=dev)
        get_poses = lambda: sim._lib.kb_get_poses(sim._h, C.c_void_p(poses.data_ptr()), sim._stream())
        poses_bytes = poses.numel() * 4
        legs = []
        for width, height in frames:
            out = torch.empty(E, height, width, 3, dtype=torch.uint8, device=dev)
            t_k, t_p = [], []
            for _ in range(args.repeats):
                t_k.append(timed(lambda: sim.render(width, height, out=out), args.launches))
                t_p.append(timed(get_poses, args.launches))
            sim.render(width, height, out=out)
            torch.cuda.synchronize()
            drawn = int((out != 255).any(-1).flatten(1).sum(1).min().item())
            assert drawn > 0, 'an env without a drawn pixel'
            want = restated(sim, width, height) if width * height <= 256 * 192 else None
            same = None if want is None else bool(np.array_equal(out[0].cpu().numpy(), want))
            assert same is not False, 'env 0 differs from the restatement'
            ms, ms_p = float(np.median(t_k)), float(np.median(t_p))
            out_bytes = out.numel()
            gbs = out_bytes / (ms * 1e-3) / 1e9
            bands = nat.render_bands(N, sim.cfg.world_width, sim.cfg.world_height, sim.cfg.bot_radius, width, height)
            legs.append({'frame': [width, height], 'bands_rows': list(bands), 'ms': round(ms, 4), 'ms_all': [round(v, 4) for v in t_k],
                         'kb_get_poses_ms': round(ms_p, 4), 'kb_get_poses_ms_all': [round(v, 4) for v in t_p],
                         'bytes_written': out_bytes, 'kb_get_poses_bytes_written': poses_bytes, 'ratio_to_kb_get_poses': round(ms / ms_p, 2),
                         'ratio_to_kb_get_poses_per_byte_written': round((ms / out_bytes) / (ms_p / poses_bytes), 2),
                         'output_gb_per_s': round(gbs, 1), 'hbm_roof_frac': round(gbs / bench.HBM_PEAK_GBS, 4),
                         'fewest_drawn_pixels_in_an_env': drawn, 'env_0_equals_the_restatement': same})
            del out
            torch.cuda.empty_cache()
        scenes.append({'scene': name, 'objects': M, 'status': status, 'legs': legs})
        sim.close()
        del sim, poses
        torch.cuda.empty_cache()
    line = {'metric': 'kb_render_ms', 'envs': E, 'bots': N, 'settle_substeps': args.settle, 'launches_per_timing': args.launches, 'repeats': args.repeats,
            'timer': 'device events around back-to-back launches, kb_render and kb_get_poses alternately, median of the repeats',
            'library': os.path.basename(nat.LIB_PATH), 'hbm_peak_gb_per_s': bench.HBM_PEAK_GBS, 'device': torch.cuda.get_device_name(0), 'scenes': scenes}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
