"""kb_sense_hops without a GPU: the symbol is exported and bound, the host-side validation answers in the header's order
(arguments before the bound check, so none of it needs a device), the kernel has no private segment and no spill (the code
object's metadata), the numpy restatement (tests/hops_ref.py) is the intended quantity -- a breadth-first search whose
parents and roots follow the header's rules, on scenes that are not vacuous -- and BatchedKilobotsEnv.hops needs comm_radius."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from tests import hops_ref as ref
from tests import reduce_ref
from tests import scenes
from tests.host_common import handle, lib  # noqa: F401
from tests.sensing_common import cloud, kernel_metadata, world_xy as world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float('nan')


def test_symbol_is_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, 'include', 'kilobots_hip.h')).read()
    assert re.search(r'\bint\s+kb_sense_hops\s*\(', hdr)
    assert 'kb_sense_hops' in nat.EXPORTS and hasattr(lib, 'kb_sense_hops')
    assert lib.kb_sense_hops.argtypes is not None and len(lib.kb_sense_hops.argtypes) == 9
    assert set(re.findall(r'\b(kb_[a-z_]+)\s*\(', hdr)) == set(nat.EXPORTS)
    assert re.search(r'#define\s+KB_HOPS_UNLIMITED\s+KB_MAX_BOTS\b', hdr)
    m = re.search(r'#define\s+KB_MAX_BOTS\s+(\d+)', hdr)
    assert m and int(m.group(1)) == nat.MAX_BOTS == nat.HOPS_UNLIMITED == ref.UNLIMITED == 1024


def test_validation_on_an_unbound_handle(lib, handle):
    """Nothing here launches: the pointers are never dereferenced on the host (any non-NULL value will do)."""
    seed, hops, par, root, stats = (C.c_void_p(0x1000 * k) for k in range(1, 6))
    bad = [
        ('NULL sim', (None, 0.07, seed, 4, hops, par, root, stats, None)),
        ('NULL d_seed', (handle, 0.07, None, 4, hops, par, root, stats, None)),
        ('NULL d_hops', (handle, 0.07, seed, 4, None, par, root, stats, None)),
        ('radius = 0', (handle, 0.0, seed, 4, hops, par, root, stats, None)),
        ('radius = -1', (handle, -1.0, seed, 4, hops, par, root, stats, None)),
        ('radius = NaN', (handle, NAN, seed, 4, hops, par, root, stats, None)),
        ('max_hops = -1', (handle, 0.07, seed, -1, hops, par, root, stats, None)),
    ]
    for what, args in bad:
        lib.kb_sense_neighbors(None, 0.07, 8, seed, seed, hops, None)     # (leaves a message that the next call must replace)
        assert lib.kb_sense_hops(*args) == nat.KB_EINVAL, what
        msg = lib.kb_last_error()
        assert msg and b'kb_sense_hops' in msg, what
    # the header's order: NULL before the radius before max_hops
    for args, word in (((handle, 0.0, None, -1, hops, None, None, None, None), b'NULL'),
                       ((handle, 0.0, seed, -1, hops, None, None, None, None), b'radius'),
                       ((handle, 0.07, seed, -1, hops, None, None, None, None), b'max_hops')):
        assert lib.kb_sense_hops(*args) == nat.KB_EINVAL and word in lib.kb_last_error(), word
    # legal arguments reach the bound check: every optional output given or NULL, max_hops 0, a radius beyond the arena
    for p in (par, None):
        for r in (root, None):
            for s in (stats, None):
                for max_hops in (0, 1, 63, nat.HOPS_UNLIMITED, 2 ** 31 - 1):
                    assert lib.kb_sense_hops(handle, 0.07, seed, max_hops, hops, p, r, s, None) == nat.KB_ENOTBOUND
                    assert b'kb_sense_hops' in lib.kb_last_error() and b'kb_bind' in lib.kb_last_error()
    assert lib.kb_sense_hops(handle, 4.0, seed, 0, hops, None, None, None, None) == nat.KB_ENOTBOUND


def test_kernel_uses_no_scratch_and_spills_nothing(lib):
    found = kernel_metadata('kb_hops_kernel')
    assert len(found) >= 1, 'no kb_hops_kernel in the code object'
    for name, fields in found:
        for key in ('.private_segment_fixed_size', '.sgpr_spill_count', '.vgpr_spill_count'):
            assert fields[key] == 0, (name, key, fields[key])


def lattice():
    return world(scenes.lattice_spawn(1, 1024, seed=3)[0][0])


def only(N, *seeds):
    s = np.zeros(N, dtype=bool)
    s[list(seeds)] = True
    return s


def check_rules(inr, seed, hop, parent, root, stats):
    """The header's rules, checked on the result itself."""
    N = len(hop)
    seed = np.asarray(seed) != 0
    assert (hop[seed] == 0).all() and (parent[seed] == -1).all() and np.array_equal(root[seed], np.flatnonzero(seed))
    out = hop < 0
    assert (hop[out] == -1).all() and (parent[out] == -1).all() and (root[out] == -1).all()
    for i in np.flatnonzero(hop > 0):
        j = parent[i]
        assert 0 <= j < N and inr[i, j] and hop[j] == hop[i] - 1, i
        assert not (inr[i, :j] & (hop[:j] == hop[i] - 1)).any(), i      # no lower index qualifies
        assert seed[root[i]] and root[i] == root[j], i
    assert stats[0] == (hop >= 0).sum() and stats[1] == hop.max(initial=-1)


def test_one_seed_is_the_breadth_first_search_of_the_reduce_tests():
    for (x, y), R in ((cloud(), 0.05), (lattice(), 0.05)):
        inr = reduce_ref.in_range(x, y, R)
        want = reduce_ref.breadth_first(inr)
        hop = ref.hops_env(inr, only(len(x), 0))[0]
        assert np.array_equal(np.where(hop < 0, np.inf, hop).astype(np.float32), want)


def test_scenes_are_not_vacuous():
    x, y = cloud()
    inr = reduce_ref.in_range(x, y, 0.05)
    hop, parent, root, stats = ref.hops_env(inr, only(333, 0))
    several = ref.candidates(inr, hop) > 1
    print('cloud: %d reached, deepest %d, %d of %d with several candidates' % (stats[0], stats[1], several.sum(), (hop > 0).sum()))
    assert stats.tolist() == [219, 15] and (hop > 0).sum() == 218 and several.sum() == 122
    check_rules(inr, only(333, 0), hop, parent, root, stats)
    x, y = lattice()
    inr = reduce_ref.in_range(x, y, 0.05)
    hop, parent, root, stats = ref.hops_env(inr, only(1024, 0))
    several = ref.candidates(inr, hop) > 1
    print('lattice: %d reached, deepest %d, %d with several candidates' % (stats[0], stats[1], several.sum()))
    assert stats.tolist() == [1024, 62] and several.sum() == 811
    check_rules(inr, only(1024, 0), hop, parent, root, stats)


def test_the_serpentine_is_a_chain():
    x, y = world(ref.serpentine())
    inr = reduce_ref.in_range(x, y, 0.045)
    assert len(x) == 1024 and inr.sum() == 2046 and inr.sum(1).max() <= 2
    hop, parent, root, stats = ref.hops_env(inr, only(1024, 0))
    assert np.array_equal(hop, np.arange(1024)) and stats.tolist() == [1024, 1023]
    assert np.array_equal(parent[1:], np.arange(1023)) and (root == 0).all()
    perm = np.random.RandomState(5).permutation(1024)
    inr_p = reduce_ref.in_range(x[perm], y[perm], 0.045)
    first = int(np.flatnonzero(perm == 0)[0])
    hop_p, parent_p, root_p, stats_p = ref.hops_env(inr_p, only(1024, first))
    assert np.array_equal(hop_p, np.arange(1024)[perm]) and stats_p.tolist() == [1024, 1023]
    check_rules(inr_p, only(1024, first), hop_p, parent_p, root_p, stats_p)


def test_permuting_the_kilobots_permutes_the_hops():
    x, y = cloud()
    seed = np.random.RandomState(6).rand(333) < 1.0 / 16
    assert 5 < seed.sum() < 60
    hop = ref.restate_env(x, y, seed, 0.05)[0]
    perm = np.random.RandomState(7).permutation(333)
    hop_p, parent_p, root_p, stats_p = ref.restate_env(x[perm], y[perm], seed[perm], 0.05)
    assert np.array_equal(hop_p, hop[perm]) and (hop > 0).any() and (hop < 0).any()
    check_rules(reduce_ref.in_range(x[perm], y[perm], 0.05), seed[perm], hop_p, parent_p, root_p, stats_p)
    assert len(np.unique(root_p[root_p >= 0])) > 3      # (several seeds own a region)


def test_max_hops_cuts_the_unlimited_result():
    x, y = cloud()
    inr = reduce_ref.in_range(x, y, 0.05)
    for seed in (only(333, 0), np.random.RandomState(6).rand(333) < 1.0 / 16):
        full = ref.hops_env(inr, seed)
        for m in (0, 1, 2, 7, 14, 15, 332, ref.UNLIMITED):
            hop, parent, root, stats = ref.hops_env(inr, seed, m)
            keep = full[0] <= m
            assert np.array_equal(hop, np.where(keep, full[0], -1)), m
            assert np.array_equal(parent, np.where(keep, full[1], -1)) and np.array_equal(root, np.where(keep, full[2], -1)), m
            assert stats.tolist() == [keep[full[0] >= 0].sum(), min(m, full[3][1])], m
    hop = ref.hops_env(inr, np.zeros(333, dtype=bool))
    assert (hop[0] == -1).all() and (hop[1] == -1).all() and (hop[2] == -1).all() and hop[3].tolist() == [0, -1]


def test_batched_env_hops_without_a_gpu():
    import torch
    from gym_kilobots_amd.envs import BatchedKilobotsEnv
    from tests.oracle_backend import OracleBackend
    env = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3)
    env.reset()
    assert env.comm_radius is None
    with pytest.raises(ValueError):
        env.hops(torch.zeros(3, 16, dtype=torch.bool))
    ok = BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3, comm_radius=0.07)
    assert ok.comm_radius == 0.07 and callable(ok.hops)
    assert torch.equal(ok.reset(), BatchedKilobotsEnv(3, 16, sim_factory=OracleBackend, seed=3).reset())
    a = torch.zeros(3, 16, 2)
    a[..., 0] = 0.01
    got, plain = ok.step(a), env.step(a)
    assert got[3] == {} and torch.equal(got[0], plain[0])       # reset() and step() gain nothing from comm_radius
