#!/usr/bin/env python3
"""Times kb_step_envs and kb_reset_envs on the settled cfg3 scene of bench.py (4096 envs x 1024 kilobots), next to kb_step.

usage: tools/bench_reset.py [--envs 4096] [--bots 1024] [--launches 20] [--repeats 10] [--out profiles/reset_envs_line.json]

Masks select every env, about one env in 8 and about one in 64, drawn at random the way the done flags of a task fall.  (A
regular stride is the worst case, not the typical one: workgroups go to the eight XCDs of the chip in turn, so every 8th or
64th env puts all selected workgroups on ONE XCD, and one env in 8 then takes as long as all of them.)  Timed in the same
process, `--repeats` times each, the order of the legs rotating from repeat to repeat so that none always follows a light one:
  kb_step                       one substep with fused actions, every env -- the yardstick;
  kb_step_envs                  the same launch with each of the three masks;
  kb_reset_envs                 each mask, without and with the step to resolve, with d_episode given (the spawn is the
                                Gaussian cloud of std 0.3 m about the centre: about 1 600 overlapping pairs per env, which the
                                default contact store holds).
Every time is the mean over `--launches` back-to-back calls between two device events after a warm-up of as many calls; the
median of the repeats is reported and all repeats kept beside it.  The steps are timed first, on the settled scene; the
resets afterwards, since they replace it.  Checked outside the timed windows: a masked step and a masked reset leave the
poses of an unselected env as they were, and the status stays clear.
KB_HIP_LIB selects another build of the library.  Prints one JSON line (and writes it to --out)."""
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
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--settle', type=int, default=120, help='substeps before the state is taken')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'reset_envs_line.json'))
    args = ap.parse_args()

    import torch
    import bench
    from gym_kilobots_amd import _native as nat
    from gym_kilobots_amd.sim import KilobotSim
    if not torch.cuda.is_available():
        sys.exit('bench_reset needs a GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    E, N = args.envs, args.bots

    def timed(fn, n):
        for _ in range(n):                      # warm-up of this shape and this load
            fn()
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
    draw = torch.rand(E, generator=torch.Generator().manual_seed(args.seed + 1)).to(dev)
    masks = {'all': torch.ones(E, dtype=torch.bool, device=dev), '1_in_8': draw < 1.0 / 8.0, '1_in_64': draw < 1.0 / 64.0}
    masks['1_in_8'][1] = masks['1_in_64'][1] = False        # (env 1 is the one that is watched)
    episode = torch.ones(E, dtype=torch.int32, device=dev)
    k = [0]

    def step(mask):
        k[0] += 1
        sim.step(1, actions=actions[k[0] % len(actions)], env_mask=mask)

    def reset(mask, resolve):
        sim.reset_envs(mask, seed=7, std=0.3, resolve=resolve, episode=episode)

    # a mask is honoured: env 1 is in neither sparse mask
    before = sim.x[1].clone()
    step(masks['1_in_8'])
    frozen = bool(torch.equal(sim.x[1], before)) and not bool(torch.equal(sim.x[0], x[0]))

    legs = [('kb_step', None)] + list(masks.items())
    t_step = {name: [] for name, _ in legs}
    for r in range(args.repeats):
        for name, m in legs[r % len(legs):] + legs[:r % len(legs)]:
            t_step[name].append(timed(lambda: step(m), args.launches))
    torch.cuda.synchronize()
    status_steps = int(sim.status.max().item())
    contacts = float(sim.ws_cnt.sum(dtype=torch.int64).item()) / E

    t_reset = {(name, r): [] for name in masks for r in (False, True)}
    legs = list(t_reset)
    for k_ in range(args.repeats):
        for (name, r) in legs[k_ % len(legs):] + legs[:k_ % len(legs)]:
            t_reset[(name, r)].append(timed(lambda: reset(masks[name], r), args.launches))
    torch.cuda.synchronize()
    before = sim.x[1].clone()
    reset(masks['1_in_64'], True)
    frozen = frozen and bool(torch.equal(sim.x[1], before))
    status_resets = int(sim.status.max().item())

    med = lambda v: round(float(np.median(v)), 4)
    ms_step = med(t_step['kb_step'])
    line = {'metric': 'kb_step_envs_and_kb_reset_envs_ms', 'envs': E, 'bots': N, 'scene': 'cfg3: settled lattice', 'settle_substeps': args.settle,
            'contacts_per_env': round(contacts, 1), 'status_after_the_steps': status_steps, 'status_after_the_resets': status_resets,
            'unselected_env_untouched': frozen, 'launches_per_timing': args.launches, 'repeats': args.repeats,
            'timer': 'device events around back-to-back calls after a warm-up of as many; the order of the legs rotates; median of the repeats',
            'masks': 'drawn at random with probability 1, 1/8 and 1/64',
            'library': os.path.basename(nat.LIB_PATH), 'device': torch.cuda.get_device_name(0),
            'kb_step_ms': ms_step, 'kb_step_ms_all': [round(v, 4) for v in t_step['kb_step']],
            'kb_step_envs': {name: {'selected_envs': int(masks[name].sum().item()), 'ms': med(t_step[name]), 'ms_all': [round(v, 4) for v in t_step[name]],
                                    'ratio_to_kb_step': round(float(np.median(t_step[name])) / float(np.median(t_step['kb_step'])), 4)} for name in masks},
            'kb_reset_envs': {'spawn_std_m': 0.3,
                              'legs': [{'mask': name, 'selected_envs': int(masks[name].sum().item()), 'resolve': r, 'ms': med(v), 'ms_all': [round(t, 4) for t in v],
                                        'ratio_to_one_kb_step': round(float(np.median(v)) / float(np.median(t_step['kb_step'])), 4)} for (name, r), v in t_reset.items()]}}
    sim.close()
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
