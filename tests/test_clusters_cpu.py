"""kb_sense_clusters without a GPU: the symbol is exported and bound, the host-side validation answers in the header's order
(arguments before the bound check, so none of it needs a device), the kernel has no private segment and no spill (the code
object's metadata), the numpy restatement (tests/clusters_ref.py) is the intended quantity -- components named by their
lowest index, whatever the numbering, with sizes, a table and stats that follow the header's rules, on scenes that are not
vacuous -- and BatchedKilobotsEnv.clusters needs comm_radius."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from tests import clusters_ref as ref
from tests import hops_ref
from tests import reduce_ref
from tests.host_common import handle, lib  # noqa: F401
from tests.sensing_common import cloud, kernel_metadata, world_xy as world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float('nan')


def test_symbol_is_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, 'include', 'kilobots_hip.h')).read()
    assert re.search(r'\bint\s+kb_sense_clusters\s*\(', hdr)
    assert 'kb_sense_clusters' in nat.EXPORTS and hasattr(lib, 'kb_sense_clusters')
    assert lib.kb_sense_clusters.argtypes is not None and len(lib.kb_sense_clusters.argtypes) == 8
    assert set(re.findall(r'\b(kb_[a-z_]+)\s*\(', hdr)) == set(nat.EXPORTS)


def test_validation_on_an_unbound_handle(lib, handle):
    """Nothing here launches: the pointers are never dereferenced on the host (any non-NULL value will do)."""
    sel, label, size, table, stats = (C.c_void_p(0x1000 * k) for k in range(1, 6))
    odd = C.c_void_p(0x4008)
    bad = [
        ('NULL sim', (None, 0.07, sel, label, size, table, stats, None)),
        ('NULL d_label', (handle, 0.07, sel, None, size, table, stats, None)),
        ('radius = 0', (handle, 0.0, sel, label, size, table, stats, None)),
        ('radius = -1', (handle, -1.0, sel, label, size, table, stats, None)),
        ('radius = NaN', (handle, NAN, sel, label, size, table, stats, None)),
        ('d_cluster off 16 bytes', (handle, 0.07, sel, label, size, odd, stats, None)),
    ]
    for what, args in bad:
        lib.kb_sense_neighbors(None, 0.07, 8, sel, sel, label, None)     # (leaves a message that the next call must replace)
        assert lib.kb_sense_clusters(*args) == nat.KB_EINVAL, what
        msg = lib.kb_last_error()
        assert msg and b'kb_sense_clusters' in msg, what
    # the header's order: NULL before the radius before the alignment
    for args, word in (((handle, 0.0, sel, None, None, odd, None, None), b'NULL'),
                       ((handle, 0.0, sel, label, None, odd, None, None), b'radius'),
                       ((handle, 0.07, sel, label, None, odd, None, None), b'16-byte')):
        assert lib.kb_sense_clusters(*args) == nat.KB_EINVAL and word in lib.kb_last_error(), word
    # legal arguments reach the bound check: the select and every optional output given or NULL, a radius beyond the arena
    for s in (sel, None):
        for sz in (size, None):
            for t in (table, None):
                for st in (stats, None):
                    assert lib.kb_sense_clusters(handle, 0.07, s, label, sz, t, st, None) == nat.KB_ENOTBOUND
                    assert b'kb_sense_clusters' in lib.kb_last_error() and b'kb_bind' in lib.kb_last_error()
    assert lib.kb_sense_clusters(handle, 4.0, None, label, None, None, None, None) == nat.KB_ENOTBOUND


def test_kernel_uses_no_scratch_and_spills_nothing(lib):
    found = kernel_metadata('kb_clusters_kernel')
    assert len(found) >= 1, 'no kb_clusters_kernel in the code object'
    for name, fields in found:
        for key in ('.private_segment_fixed_size', '.sgpr_spill_count', '.vgpr_spill_count'):
            assert fields[key] == 0, (name, key, fields[key])


def check_rules(inr, x, y, select, label, size, table, stats):
    """The header's rules, checked on the result itself."""
    N = len(label)
    sel = np.ones(N, dtype=bool) if select is None else np.asarray(select) != 0
    assert (label[~sel] == -1).all() and (size[~sel] == 0).all() and (label[sel] >= 0).all()
    assert (label[sel] <= np.flatnonzero(sel)).all() and (label[label[sel]] == label[sel]).all()
    m = inr & sel[:, None] & sel[None, :]
    i, j = np.nonzero(m)
    assert (label[i] == label[j]).all()                     # an edge never leaves a component
    roots = np.flatnonzero(label == np.arange(N))
    for r in roots:
        mem = label == r
        assert not m[mem][:, sel & ~mem].any()              # closed: nothing outside is in range of a member
        assert (size[mem] == mem.sum()).all() and table[r, 0] == mem.sum()
        assert np.flatnonzero(mem)[0] == r
    assert size[sel].sum() == sum(int((label == r).sum()) ** 2 for r in roots) and table[:, 0].sum() == sel.sum()
    rest = np.ones(N, dtype=bool)
    rest[roots] = False
    assert (table[rest].view(np.uint32) == 0).all()         # every other row is four +0.0f
    sizes = np.array([(label == r).sum() for r in roots], dtype=np.int64)
    if len(roots):
        big = sizes.max()
        assert stats.tolist() == [len(roots), big, roots[sizes == big][0], (sizes == 1).sum()]
    else:
        assert stats.tolist() == [0, 0, -1, 0]


def test_scenes_are_not_vacuous():
    x, y = cloud()
    inr = reduce_ref.in_range(x, y, 0.05)
    label, size, table, stats = ref.clusters_env(inr, x, y)
    print('cloud: %s' % stats.tolist())
    assert stats[0] >= 2 and stats[1] >= 3 and stats[3] >= 1 and stats[1] == 219 and stats[2] == 0
    check_rules(inr, x, y, None, label, size, table, stats)
    select = np.random.RandomState(21).rand(333) < 0.75
    got = ref.clusters_env(inr, x, y, select)
    print('cloud, 3 in 4: %s' % got[3].tolist())
    assert got[3][0] >= 2 and got[3][1] >= 3 and got[3][3] >= 1 and not np.array_equal(got[0], label)
    check_rules(inr, x, y, select, *got)
    # uint8 bytes that are not 1 select as well
    assert all(np.array_equal(a, b) for a, b in zip(got, ref.clusters_env(inr, x, y, select.astype(np.uint8) * 0xFF)))


def test_permuting_the_kilobots_maps_a_label_to_the_lowest_permuted_index():
    x, y = cloud()
    label = ref.restate_env(x, y, 0.05)[0]
    perm = np.random.RandomState(7).permutation(333)        # kilobot i of the permuted scene is kilobot perm[i]
    label_p, size_p, table_p, stats_p = ref.restate_env(x[perm], y[perm], 0.05)
    old = label[perm]                                       # the old label of every permuted kilobot names its component
    want = np.array([np.flatnonzero(old == c)[0] for c in old], dtype=np.int32)
    assert np.array_equal(label_p, want) and not np.array_equal(label_p, old)
    size = ref.restate_env(x, y, 0.05)[1]
    assert np.array_equal(size_p, size[perm])
    assert stats_p[[0, 1, 3]].tolist() == ref.restate_env(x, y, 0.05)[3][[0, 1, 3]].tolist()
    # the table is exact on the quantised values and independent of any order: the same bits under the new label
    table = ref.restate_env(x, y, 0.05)[2]
    for r in np.flatnonzero(label == np.arange(333)):
        assert np.array_equal(table[r].view(np.uint32), table_p[want[np.flatnonzero(perm == r)[0]]].view(np.uint32))


def test_a_larger_radius_only_merges():
    x, y = cloud()
    radii = (0.034, 0.05, 0.07, 0.1, 0.3)
    labels = [ref.restate_env(x, y, R) for R in radii]
    for (small, _, _, ss), (big, _, _, sb) in zip(labels, labels[1:]):
        assert np.array_equal(big[small], big) and (big <= small).all()         # a component goes whole into one component
        assert sb[0] <= ss[0] and sb[1] >= ss[1] and sb[3] <= ss[3]
    assert labels[0][3][0] > labels[1][3][0] > labels[2][3][0] > 1 and labels[-1][3].tolist() == [1, 333, 0, 0]


def test_sizes_sum_to_the_selected():
    x, y = cloud()
    inr = reduce_ref.in_range(x, y, 0.05)
    for select in (None, np.random.RandomState(21).rand(333) < 0.75, np.zeros(333, dtype=bool), np.arange(333) == 17):
        label, size, table, stats = ref.clusters_env(inr, x, y, select)
        n = 333 if select is None else int(select.sum())
        roots = label == np.arange(333)
        assert size[roots].sum() == n and table[:, 0].sum() == n and (label >= 0).sum() == n
    assert stats.tolist() == [1, 1, 17, 1] and label[17] == 17
    assert ref.clusters_env(inr, x, y, np.zeros(333))[3].tolist() == [0, 0, -1, 0]


def test_the_row_of_an_isolated_kilobot():
    """n = 1: the centroid is the kilobot's QUANTISED position, ((float)q / 1) / 65536, and the extent is the distance of the
    kilobot from it: not zero in general, the quantum 2^-16 drops the last bits of a coordinate beyond 1 world unit, but never
    more than the half quantum in either coordinate allows."""
    x, y = cloud()
    label, size, table, stats = ref.restate_env(x, y, 0.05)
    alone = np.flatnonzero(size == 1)
    assert len(alone) == stats[3] >= 1 and (label[alone] == alone).all()
    for b in alone:
        qx, qy = ref.quant(x[b:b + 1])[0], ref.quant(y[b:b + 1])[0]
        cxw, cyw = np.float32(qx) / np.float32(65536), np.float32(qy) / np.float32(65536)
        assert abs(float(cxw) - float(x[b])) <= 2.0 ** -17 and abs(float(cyw) - float(y[b])) <= 2.0 ** -17
        ex, ey = x[b] - cxw, y[b] - cyw
        want = np.array([1.0, cxw / np.float32(25), cyw / np.float32(25), np.sqrt(ex * ex + ey * ey) / np.float32(25)], dtype=np.float32)
        assert np.array_equal(table[b].view(np.uint32), want.view(np.uint32))
        assert table[b, 3] <= 2.0 ** -16 / 25.0
    assert (table[alone, 3] > 0).any()


def test_one_seed_per_component_gives_the_roots_of_hops():
    x, y = cloud()
    inr = reduce_ref.in_range(x, y, 0.05)
    label = ref.labels_env(inr)
    seeds = label == np.arange(333)
    hop, parent, root, stats = hops_ref.hops_env(inr, seeds)
    assert np.array_equal(root, label) and stats[0] == 333 and seeds.sum() >= 2


def test_the_serpentine():
    x, y = world(hops_ref.serpentine())
    inr = reduce_ref.in_range(x, y, 0.045)
    label, size, table, stats = ref.clusters_env(inr, x, y)
    assert (label == 0).all() and (size == 1024).all() and stats.tolist() == [1, 1024, 0, 0]
    select = np.arange(1024) % 64 != 63
    label, size, table, stats = ref.clusters_env(inr, x, y, select)
    assert np.array_equal(label, np.where(select, np.arange(1024) // 64 * 64, -1))
    assert np.array_equal(size, np.where(select, 63, 0)) and stats.tolist() == [16, 63, 0, 0]
    check_rules(inr, x, y, select, label, size, table, stats)
    # permuted: the chain position pos[i] of kilobot i; a run of the chain is named by the lowest index in it
    pos = np.random.RandomState(5).permutation(1024)
    inr_p = reduce_ref.in_range(x[pos], y[pos], 0.045)
    sel_p = pos % 64 != 63
    label_p, size_p, table_p, stats_p = ref.clusters_env(inr_p, x[pos], y[pos], sel_p)
    lowest = {run: int(np.flatnonzero((pos // 64 == run) & sel_p)[0]) for run in range(16)}
    assert np.array_equal(label_p, np.where(sel_p, [lowest[r] for r in pos // 64], -1))
    assert stats_p.tolist() == [16, 63, min(lowest.values()), 0]
    assert (ref.clusters_env(inr_p, x[pos], y[pos])[0] == 0).all()


def test_batched_env_clusters_without_a_gpu():
    import torch
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    from tests.oracle_backend import OracleBackend
    env = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3)
    env.reset()
    assert env.comm_radius is None
    with pytest.raises(ValueError):
        env.clusters()
    with pytest.raises(ValueError):
        env.clusters(torch.ones(3, 16, dtype=torch.bool), stats=True)
    ok = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3, comm_radius=0.07)
    assert ok.comm_radius == 0.07 and callable(ok.clusters)
    assert torch.equal(ok.reset(), BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3).reset())
