"""The island placement of the register solver in the kernels without objects (kb_step_kernel.h, "Placement of the islands on
the waves in order of size"), as tools/placement_model.py states it: next-fit packing that closes a wave at one register slot
(64 contacts) while the rest still fits the waves behind it at 128, with the even split as the fallback.  Checked on random
multisets of island sizes and on hand-made edge cases, for 2, 4 and 8 sweeping waves: every island on one wave, a one-slot wave
within 64, no wave above 128 where the even split stays within it, the two-slot waves last, nothing depends on the order inside
a size class -- and the wave starts the kernel computes from the class totals give the wave the sequential walk gives."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import placement_model as PM  # noqa: E402

WAVES = (2, 4, 8)


def worst_waste(nw, s):
    """islands of s contacts that leave s - 1 (or the most possible) unused at every boundary of 64 and of 128"""
    return [s] * (nw * (PM.WAVE // s))


def cases(nw):
    rng = random.Random(1234 + nw)
    out = [
        ('all ones', [1] * (50 * nw)),
        ('all ones, full', [1] * (128 * nw)),
        ('one of 65', [65] + [1] * 20 + [2] * 10),
        ('one of 128', [128] + [3] * 8 + [1] * 30),
        ('one of 31', [31] + [1] * (60 * nw)),
        ('exactly 64 nw', [16] * (4 * nw)),
        ('exactly 64 nw in ones', [1] * (64 * nw)),
        ('exactly 64 (nw - 1) + 128', [8] * (8 * (nw - 1) + 16)),
        ('exactly 128 nw', [4] * (32 * nw)),
        ('one past 128 nw', [4] * (32 * nw) + [1]),
        ('nothing', []),
        ('one contact', [1]),
    ]
    for s in (3, 5, 7, 9, 13, 17, 23, 29, 31):
        out.append(('waste of %d' % s, worst_waste(nw, s)))
        out.append(('waste of %d, then ones' % s, [s] * (nw * (PM.SLOT // s) // 2) + [1] * (30 * nw)))
        out.append(('waste of %d over 64 (nw - 1)' % s, [s] * ((nw - 1) * (PM.SLOT // s) + 1)))
    for k in range(300):
        top = rng.choice((2, 4, 8, 16, 31, 31, 40))
        total = rng.randint(1, 140 * nw)
        sizes = []
        while sum(sizes) < total:
            sizes.append(min(rng.randint(1, top), rng.randint(1, top)))
        rng.shuffle(sizes)
        out.append(('random %d' % k, sizes))
    return out


@pytest.mark.parametrize('nw', WAVES)
def test_packed_placement(nw):
    packed = fallbacks = 0
    for name, sizes in cases(nw):
        what = '%s on %d waves: %s' % (name, nw, sizes)
        waves, rule = PM.place(sizes, nw)
        # every island on exactly one wave, and the counts add up
        assert len(waves) == len(sizes) and all(0 <= w < nw for w in waves), what
        load = PM.loads(sizes, waves, nw)
        assert sum(load) == sum(sizes), what
        even = PM.loads(sizes, PM.even_split(sizes, nw), nw)
        walk = PM.packed_walk(sizes, nw)
        if rule == 'even':
            fallbacks += 1
            # the fallback is the even split itself; it is taken for an island of 32 and more, or where the walk runs out of waves
            assert load == even, what
            assert walk is None and (max(sizes) >= PM.CLASSES or sum(sizes) > 0), what
            if max(sizes) < PM.CLASSES:
                assert max(even) > PM.WAVE, what + ': the packing ran out of waves where the even split %s does not' % even
            continue
        packed += 1
        two = walk[1]
        assert max(sizes, default=0) < PM.CLASSES, what
        # a wave closed at one slot holds at most 64, none more than 128
        assert all(c <= PM.SLOT for c in load[:two]), what + ': %s, two-slot from wave %d' % (load, two)
        assert all(c <= PM.WAVE for c in load), what + ': %s' % load
        # the two-slot waves come behind the one-slot waves in the walk
        over = [w for w, c in enumerate(load) if c > PM.SLOT]
        assert all(w >= two for w in over), what
        used = [w for w, c in enumerate(load) if c]
        assert used == list(range(len(used))), what + ': a wave is skipped, %s' % load
        # the walk goes down the sizes: no island on an earlier wave than a larger one
        order = PM.walk_order(sizes)
        assert all(waves[a] <= waves[b] for a, b in zip(order, order[1:])), what
        # never worse than the even split where that stays on the register path
        if max(even, default=0) <= PM.WAVE:
            assert max(load, default=0) <= PM.WAVE, what
    assert packed > 100 and fallbacks > 10, (packed, fallbacks)


@pytest.mark.parametrize('nw', WAVES)
def test_order_inside_a_size_class_does_not_matter(nw):
    rng = random.Random(99 + nw)
    for name, sizes in cases(nw):
        if any(s >= PM.CLASSES for s in sizes):
            continue        # (class 0 is of mixed sizes: the even split it takes is exact up to the order of those islands)
        ref = PM.place(sizes, nw)
        ref_loads = PM.loads(sizes, ref[0], nw)
        for _ in range(3):
            perm = list(range(len(sizes)))
            rng.shuffle(perm)
            shuffled = [sizes[i] for i in perm]
            got = PM.place(shuffled, nw)
            assert got[1] == ref[1], name
            assert PM.loads(shuffled, got[0], nw) == ref_loads, '%s on %d waves' % (name, nw)
            # ... and the islands of a class are spread over the waves in the same numbers
            per = lambda sz, wv: sorted(zip(sz, wv))        # noqa: E731
            assert per(shuffled, got[0]) == per(sizes, ref[0]), name


@pytest.mark.parametrize('nw', WAVES)
def test_wave_starts_are_the_sequential_walk(nw):
    """the form the kernel computes -- one step per wave over the class totals, then every island by the place of its first
    contact -- against the walk over the islands"""
    for name, sizes in cases(nw):
        what = '%s on %d waves: %s' % (name, nw, sizes)
        walk, table = PM.packed_walk(sizes, nw), PM.table_walk(sizes, nw)
        assert (walk is None) == (table is None), what
        if walk is not None:
            assert walk == table, what
            starts, counts, two = PM.wave_starts(sizes, nw)
            assert counts == PM.loads(sizes, walk[0], nw) and two == walk[1], what
            assert starts[0] == 0 and starts == sorted(starts) and starts[-1] <= sum(sizes), what


def test_division_by_an_island_size():
    for s in range(1, PM.CLASSES + 1):
        for x in range(PM.WAVE + 1):
            assert (x * PM.magic(s)) >> 16 == x // s, (x, s)


def test_the_headline_shape():
    """about 550 contacts in islands of a few contacts on eight waves: the first six waves (at least) hold one slot, filled
    but for the waste of an island of twelve, and at most two waves at the end take two"""
    rng = random.Random(7)
    sizes = []
    while sum(sizes) < 548:
        sizes.append(rng.choice((1, 1, 1, 2, 2, 3, 4, 5, 7, 9, 12)))
    waves, rule = PM.place(sizes, 8)
    load = PM.loads(sizes, waves, 8)
    assert rule == 'packed'
    assert all(53 <= c <= 64 for c in load[:6]) and all(c <= 128 for c in load[6:]), load
    assert 1 <= sum(1 for c in load if c > 64) <= 2, load
    even = PM.loads(sizes, PM.even_split(sizes, 8), 8)
    assert sum(1 for c in even if c > 64) >= 6, even
