#!/usr/bin/env python3
"""Island placement of the register solver in the kernels without objects, stated in Python and priced on the oracle (no GPU).

The kernel (kb_step_kernel.h, "Placement of the islands on the waves in order of size") walks the islands of an env by size
class -- class q holds the islands of 32 - q contacts, class 0 those of 32 and more; inside a class the order is whatever the
atomics give -- and puts them on the `nw` sweeping waves.  A lane of a wave holds KB_KREG_BINS = 2 contacts: 64 contacts are one
register slot, 128 are a wave.  Two rules:

    even split   (the kernels up to here; still the fallback) consecutive stretches of ceil(ncon / nw) contacts, an island goes
                 to the wave its first contact falls on
    packed       next fit in walk order.  A wave that is opened gets a capacity, 64 or 128, and is closed by the first island
                 that does not fit the room left in it.  It gets 64 as long as what is still unplaced fits the waves behind
                 it at 128 each, reckoning for every wave the most it can waste: the size s of the largest island left, minus
                 one.  With R contacts unplaced when wave w is opened: 64 iff R - (65 - s) <= (nw - 1 - w) * (129 - s).  From the
                 first wave where that fails on, every wave gets 128: the two-slot waves come last, among the smallest islands.
                 An env with an island of 32 contacts or more, or whose walk runs out of waves, takes the even split instead
                 (if the walk runs out of waves at 128 each, the even split overloads a wave as well: next fit closes every
                 wave no earlier than the even split does).

`packed_walk` is that rule as a sequential walk over the islands.  `wave_starts` / `wave_from_starts` are the form the kernel
computes: wave 0 walks over the 31 class totals, one step per wave, and leaves the first contact of every wave (counted in walk
order) and the contacts per wave; every island then finds its wave from the place of its first contact, which is the start of
its class plus its index within the class times the class's size.  tests/test_placement_cpu.py holds the two forms equal.

Run as a program it settles bench.py's scene on the oracle, rebuilds every env's contacts from the packed warm-start list,
orders them canonically, counts depth levels as the kernel's depth pass does, and prints for both rules the two-slot waves per
env and the rounds one sweep of the slowest wave runs (the distinct levels among a wave's 64 shallowest contacts plus the
distinct levels among the rest: a level split over the two slots is swept in two rounds).

    python tools/placement_model.py [--envs 24 --bots 1024 --substeps 130 --waves 8]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLOT = 64               # contacts of one register slot of a wave (one per lane)
WAVE = 128              # 64 * KB_KREG_BINS: contacts a wave can hold
CLASSES = 32            # size classes; class 0: 32 contacts and more
RK = 4                  # kb_launch.h: rank buckets per class (the depth pass goes rank by rank in the last one, as here everywhere)


def size_class(s):
    return CLASSES - min(int(s), CLASSES)


def walk_order(sizes):
    """indices of the islands in walk order: by size class, inside a class as given"""
    return sorted(range(len(sizes)), key=lambda i: size_class(sizes[i]))


def loads(sizes, waves, nw):
    out = [0] * nw
    for s, w in zip(sizes, waves):
        out[w] += int(s)
    return out


def even_split(sizes, nw):
    """wave of every island under the even split"""
    ncon = int(sum(sizes))
    chunk = max((ncon + nw - 1) // nw, 1)
    waves, at = [0] * len(sizes), 0
    for i in walk_order(sizes):
        waves[i] = min(at // chunk, nw - 1)
        at += int(sizes[i])
    return waves


def one_slot(unplaced, s, w, nw):
    """may wave w, opened with `unplaced` contacts left of which the largest island has s, be closed at 64?"""
    return unplaced - (SLOT + 1 - s) <= (nw - 1 - w) * (WAVE + 1 - s)


def packed_walk(sizes, nw):
    """(wave of every island, first two-slot wave [nw: none]) of the packed rule, or None where the env takes the even split"""
    if any(s >= CLASSES for s in sizes):
        return None
    total, placed = int(sum(sizes)), 0
    waves = [0] * len(sizes)
    w, room, two = -1, 0, nw
    for i in walk_order(sizes):
        s = int(sizes[i])
        if s > room:
            w += 1
            if w == nw:
                return None
            if two == nw and not one_slot(total - placed, s, w, nw):
                two = w
            room = SLOT if w < two else WAVE
        waves[i] = w
        room -= s
        placed += s
    return waves, two


def magic(s):
    """x // s == (x * magic(s)) >> 16 for 0 <= x <= 128 and 1 <= s <= 32: the kernel's division by an island size"""
    return 65536 // s + 1


def wave_starts(sizes, nw):
    """What wave 0 of the kernel leaves, from the class totals alone: (first contact of every wave, counted in walk order,
    contacts per wave, first two-slot wave [nw: none]), or None where the env takes the even split.  One step per wave: the
    wave takes every class that still fits as a whole, and of the first class that does not as many islands as fit."""
    held = [0] * CLASSES
    for s in sizes:
        held[size_class(s)] += int(s)
    if held[0]:
        return None
    incl = list(np.cumsum(held))
    excl = [i - h for i, h in zip(incl, held)]
    total = incl[-1]
    starts, counts = [total] * nw, [0] * nw
    starts[0] = 0
    pos, two = 0, nw
    for w in range(nw):
        if pos >= total:
            break
        s = CLASSES - min(q for q in range(CLASSES) if incl[q] > pos)       # the largest island left
        if two == nw and not one_slot(total - pos, s, w, nw):
            two = w
        end = pos + (SLOT if w < two else WAVE)
        over = [q for q in range(CLASSES) if incl[q] > end]                 # the classes that do not fit as a whole
        nxt = total
        if over:
            q = over[0]
            start = max(pos, excl[q])
            assert 0 <= end - start <= WAVE
            nxt = start + (((end - start) * magic(CLASSES - q)) >> 16) * (CLASSES - q)
        if w + 1 < nw:
            starts[w + 1] = nxt
        counts[w] = nxt - pos
        pos = nxt
    if pos < total:
        return None
    return starts, counts, two


def wave_from_starts(starts, at):
    """wave of the island whose first contact is number `at` of the walk"""
    return sum(1 for k in range(1, len(starts)) if at >= starts[k])


def table_walk(sizes, nw):
    """the packed rule as the kernel computes it: (waves, first two-slot wave) or None.  An island's first contact is its
    class's start plus the contacts of the islands of the class that came before it (any order: they are of one size)."""
    table = wave_starts(sizes, nw)
    if table is None:
        return None
    held = [0] * CLASSES
    for s in sizes:
        held[size_class(s)] += int(s)
    at = [int(v) for v in np.cumsum(held) - held]
    waves = [0] * len(sizes)
    for i in walk_order(sizes):
        q = size_class(sizes[i])
        waves[i] = wave_from_starts(table[0], at[q])
        at[q] += int(sizes[i])
    assert loads(sizes, waves, nw) == table[1], (sizes, table)
    return waves, table[2]


def place(sizes, nw):
    """(wave of every island, 'packed' | 'even'): what the kernel does"""
    got = packed_walk(sizes, nw)
    if got is None:
        return even_split(sizes, nw), 'even'
    return got[0], 'packed'


# ---- the contacts of an env, from the oracle's packed list and the poses the substep started from ------------------------------
CELL, XMIN, YMIN, GW, GH = 0.875, -25.0, -18.75, 58, 43          # world units (kb_common.h: CELL_SIZE; the 2 x 1.5 m arena)
WALL_KEY = 0x10000
DIRS = {(0, 0): 0, (1, 0): 1, (0, 1): 3, (1, 1): 5, (-1, 1): 7}          # oracle/kb_oracle.c: CLS_SAME, CLS_E, CLS_N, CLS_NE, CLS_NW
CLS_WALL = 9


def env_contacts(x, y, ws_key, ws_cnt):
    """[(class, rank, A, B)] in canonical order; A < 0: wall -1 - A.  Sorted by (class, group, A, B), the rank counts inside
    a (class, group)."""
    N = len(ws_cnt)
    cx = np.clip(np.floor((x.astype(np.float32) - np.float32(XMIN)) * np.float32(1.0 / CELL)).astype(np.int64), 0, GW - 1)
    cy = np.clip(np.floor((y.astype(np.float32) - np.float32(YMIN)) * np.float32(1.0 / CELL)).astype(np.int64), 0, GH - 1)
    owner = np.repeat(np.arange(N), np.asarray(ws_cnt).astype(np.int64))
    key = np.asarray(ws_key)[:len(owner)].astype(np.int64)
    rows = []
    for a, k in zip(owner, key):
        a, k = int(a), int(k)
        if k >= WALL_KEY:
            rows.append((CLS_WALL, a, -1 - (k - WALL_KEY), a))
            continue
        d = (int(cx[k] - cx[a]), int(cy[k] - cy[a]))
        cls = DIRS[d]
        if d[0] != 0:
            cls += int(cx[a]) & 1
        elif d[1] != 0:
            cls += int(cy[a]) & 1
        rows.append((cls, int(cy[a]) * GW + int(cx[a]), a, k))
    rows.sort()
    out, rank, prev = [], 0, None
    for cls, grp, a, b in rows:
        rank = rank + 1 if (cls, grp) == prev else 0
        prev = (cls, grp)
        out.append((cls, rank, a, b))
    return out


def islands_and_depths(contacts, N):
    """(island root per contact, depth level per contact): the sweep order is (class, rank); a contact's level is one more
    than the level of the latest earlier contact on either of its bodies"""
    parent = list(range(N))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for _, _, a, b in contacts:
        if a >= 0:
            parent[find(a)] = find(b)
    order = sorted(range(len(contacts)), key=lambda i: contacts[i][:2])
    body = [0] * N
    depth = [0] * len(contacts)
    for i in order:
        _, _, a, b = contacts[i]
        d = max(body[a] if a >= 0 else 0, body[b]) + 1
        depth[i] = d
        body[b] = d
        if a >= 0:
            body[a] = d
    return [find(b) for _, _, _, b in contacts], depth


def sweep_rounds(levels):
    """rounds of one sweep of a wave whose contacts have these depth levels"""
    lv = sorted(levels)
    return len(set(lv[:SLOT])) + len(set(lv[SLOT:]))


def env_report(contacts, N, nw, rule):
    """(contacts per wave, rounds per sweep per wave) of one env under rule 'even' | 'packed'"""
    root, depth = islands_and_depths(contacts, N)
    roots = sorted(set(root))
    sizes = [root.count(r) for r in roots]
    waves = even_split(sizes, nw) if rule == 'even' else place(sizes, nw)[0]
    of = dict(zip(roots, waves))
    levels = [[] for _ in range(nw)]
    for r, d in zip(root, depth):
        levels[of[r]].append(d)
    return [len(l) for l in levels], [sweep_rounds(l) for l in levels]


def settled_envs(E, N, substeps):
    """bench.py's scene on the oracle: (x, y of the poses the last substep started from, ws_key, ws_cnt after it)"""
    import torch
    import bench
    from oracle import oracle as O
    x, y, th, acts = bench.make_scene(torch, E, N, torch.device('cpu'), 0, 0, 0)
    osim = O.OracleSim(O.default_config(E, N, allow_sleep=0))
    osim.x[...] = x.numpy()
    osim.y[...] = y.numpy()
    osim.theta[...] = th.numpy()
    x0 = y0 = None
    for k in range(substeps):
        x0, y0 = osim.x.copy(), osim.y.copy()
        osim.set_actions(acts[k % len(acts)].numpy())
        osim.step(1, threads=min(E, os.cpu_count() or 1, 16))
    return x0, y0, osim.ws_key, osim.ws_cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=24)
    ap.add_argument('--bots', type=int, default=1024)
    ap.add_argument('--substeps', type=int, default=130)
    ap.add_argument('--waves', type=int, default=8)
    args = ap.parse_args()
    E, N, nw = args.envs, args.bots, args.waves
    x, y, key, cnt = settled_envs(E, N, args.substeps)
    ncon = cnt.astype(np.int64).sum(1)
    print('%d envs x %d kilobots, %d substeps: %.1f contacts per env (%d .. %d)' % (E, N, args.substeps, ncon.mean(), ncon.min(), ncon.max()))
    res = {}
    for rule in ('even', 'packed'):
        two, slow, first = [], [], None
        for e in range(E):
            con = env_contacts(x[e], y[e], key[e], cnt[e])
            per_wave, rounds = env_report(con, N, nw, rule)
            two.append(sum(1 for c in per_wave if c > SLOT))
            slow.append(max(rounds))
            assert max(per_wave) <= WAVE, per_wave
            if first is None:
                first = (per_wave, rounds)
        res[rule] = (np.mean(two), np.mean(slow), first)
    print('%-44s %-26s %s' % ('', 'even split', 'next-fit packing at 64'))
    print('%-44s %-26s %s' % ('waves with two slots, per env', '%.2f of %d' % (res['even'][0], nw), '%.2f of %d' % (res['packed'][0], nw)))
    print('%-44s %-26s %s' % ('rounds per sweep, slowest wave', '%.2f' % res['even'][1], '%.2f' % res['packed'][1]))
    print('%-44s %-26s %s' % ('contacts per wave, env 0', ' '.join(map(str, res['even'][2][0])), ' '.join(map(str, res['packed'][2][0]))))
    print('%-44s %-26s %s' % ('rounds per sweep per wave, env 0', ' '.join(map(str, res['even'][2][1])), ' '.join(map(str, res['packed'][2][1]))))


if __name__ == '__main__':
    main()
