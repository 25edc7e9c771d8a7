"""The contact-count regimes of the solver in the step kernels without objects, and scenes that visit each of them.

The kernel chooses the path of a substep's contact solve per env from the number of contacts `ncon` of that substep
(kb_step_kernel.h: `big = newTotal + extras > capS`, `reg = ... maxw <= 64u * KRX`, the last line of the solver selection
`if (BINS && nw > 1 && !reg && p.solver_mode == 0) coop = true`; kb_coopsolve_bins.inc: `accInLds`).  With nw waves per
workgroup (kb_block_threads / 64), capL = kb_lds_staging_entries and cap = kb_contact_capacity:

    R0   ncon <= 128              register solver (kb_regsolve_bins.inc): no wave can hold more than 64 lanes x KB_KREG_BINS
                                  contacts, and no island exceeds GIANT_ISLAND
    R1   128 nw < ncon <= capL    cooperative level sweep, contacts staged in LDS, impulses in LDS
    R2   capL < ncon <= 3 capL    cooperative sweep, contacts staged in the global slice, impulses in LDS
    R3   3 capL < ncon <= cap     cooperative sweep, global slice, impulses kept in the global records

Between 128 and 128 nw contacts the path depends on how the islands fall onto the waves, and above cap the list is cut
(status bit 0): `regime` answers None there -- undecided from outside.  ncon of a substep is ws_cnt.sum(axis=1) after it,
as long as the status word is 0 (a contact beyond the warm-start slots of its owner is solved but not stored, and
flagged).

Shared by tests/test_solver_regimes_cpu.py (every scene visits on the oracle exactly the regimes its row claims, with
the band limits read through the ABI: the guard against a vacuous device test) and tests/test_solver_regimes_gpu.py
(every substep of every scene bit for bit against the oracle, classified from the device's own counts)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

from oracle import oracle as O
from tests import scenes
from tests.scenes import scene_id  # noqa: F401

LANES = 64
KREG_BINS = 2               # kb_common.h: KB_KREG_BINS, contacts a lane of the register solver holds
REG_CONTACTS = LANES * KREG_BINS        # = GIANT_ISLAND / 2 (kb_common.h: GIANT_ISLAND = 256): an env that fits R0 has no giant island
GIANT_ISLAND = 256
ACC_LDS_FACTOR = 3          # kb_coopsolve_bins.inc: accInLds = ncon <= (big ? 3 * capL_ : capL_)
NCELL = 2494                # broadphase cells of the 2 x 1.5 m arena (tests/test_launch_cpu.py: ARENAS)


def regime(ncon, nw, capL, cap):
    """'R0' | 'R1' | 'R2' | 'R3', or None where the count alone does not decide the path."""
    if ncon <= REG_CONTACTS:
        return 'R0'
    if ncon <= REG_CONTACTS * nw or ncon > cap:
        return None
    if ncon <= capL:
        return 'R1'
    if ncon <= ACC_LDS_FACTOR * capL:
        return 'R2'
    return 'R3'


def counts(ws_cnt):
    """ncon of the last substep per env, from a [E, N] ws_cnt array"""
    return np.asarray(ws_cnt).astype(np.int64).sum(axis=1)


# The scenes: scenes.lattice_spawn(E, N, SEED, pitch, jitter=JITTER) on pitches below the kilobot diameter (0.033 m), every
# kilobot driven with scenes.random_actions, DRIVE_VELOCITY, no light, solver_mode 0.  An overlapping lattice is pushed apart
# within a few substeps and passes through the regimes on its way down; a lattice just above the diameter closes up under
# the random drive and climbs through R0.
#   visits     regime -> the least number of substeps (of every env) in it; the set of keys is what the scene visits, exactly
#   gap        substeps with an undecided count (128 < ncon <= 128 nw) occur as well
# Band limits of the default 2 x 1.5 m arena, for orientation (the tests read them through the ABI):
#   N = 200: nw 2, capL 280, cap 2304;  N = 256, capacity 4096: nw 4, capL 832;  N = 640, capacity 4096: nw 8, capL 1024;
#   N = 1024 (fixed-size kernel): nw 8, capL 688, cap 4160.
# At 1024 kilobots 128 nw = 1024 > capL = 688: R1 cannot be told by count there, so no row claims it.
# At 200 kilobots R1 is the narrow band 257 .. 280; the lattice on 0.033 m settles inside it (257 .. 272 contacts).
SEED, JITTER = 3, 0.002
_S = lambda name, N, capacity, pitch, substeps, visits, gap=False: SimpleNamespace(   # noqa: E731
    name=name, N=N, capacity=capacity, pitch=pitch, substeps=substeps, visits=visits, gap=gap)
SCENES = [
    _S('200-p014', 200, 0, 0.014, 12, {'R3': 2, 'R2': 8}),
    _S('200-p033', 200, 0, 0.033, 14, {'R1': 8}, gap=True),
    _S('200-p036', 200, 0, 0.036, 12, {'R0': 12}),
    _S('256-p010', 256, 4096, 0.010, 14, {'R3': 1, 'R2': 6, 'R1': 4}),
    _S('256-p036', 256, 4096, 0.036, 10, {'R0': 10}),
    _S('640-p016', 640, 4096, 0.016, 6, {'R3': 2, 'R2': 3}),
    _S('1024-p022', 1024, 0, 0.022, 12, {'R3': 12}),
    _S('1024-p030', 1024, 0, 0.030, 12, {'R2': 6, 'R3': 3}),
    _S('1024-p042', 1024, 0, 0.042, 12, {'R0': 12}),
]
REPLICA_SCENE = SCENES[6]       # the CU-filling replicas: R3 in every substep
REPLICA_ENVS = 4                # distinct envs that are tiled
R0_MIN_CONTACTS = 64            # an R0 scene must reach this many contacts (more than one per lane), not rest at none
FUSED_SUBSTEPS = 10


def config_kw(s, allow_sleep):
    return dict(allow_sleep=allow_sleep, contact_capacity=s.capacity, solver_mode=0)


def plan_inputs(N, capacity, allow_sleep):
    """The eleven inputs of plan_launch (columns of tests/golden/launch_plan.txt) of a scene here."""
    return [N, 0, 0, 0, O.DRIVE_VELOCITY, O.LIGHT_NONE, 0, allow_sleep, NCELL, capacity, 0]


def start(s, E, seed=SEED):
    """seed: another one gives the twin scene of tests/guarded.py -- the same lattice with other jitter and headings"""
    return scenes.lattice_spawn(E, s.N, seed, s.pitch, jitter=JITTER)


def actions(E, N, k):
    return scenes.random_actions(E, N, seed=100 + k)


def bands(lib, nat, N, capacity, allow_sleep):
    """(nw, capL, cap) of the handle kb_create makes of the configuration -- no GPU needed."""
    cfg = nat.default_config(1, N, O.DRIVE_VELOCITY, O.LIGHT_NONE, contact_capacity=capacity, allow_sleep=allow_sleep)
    h = C.c_void_p()
    rc = lib.kb_create(C.byref(cfg), C.byref(h))
    assert rc == nat.KB_OK, rc
    out = (lib.kb_block_threads(h) // LANES, lib.kb_lds_staging_entries(h), lib.kb_contact_capacity(h))
    lib.kb_destroy(h)
    return out


def classify(ws_cnt, band):
    return [regime(int(n), *band) for n in counts(ws_cnt)]


def check_visits(s, seen, what=''):
    """seen: per substep the list of regimes per env.  Every env visits exactly the regimes of the row, each for at least
    the row's number of substeps; undecided counts only where the row says so."""
    E = len(seen[0])
    for e in range(E):
        col = [r[e] for r in seen]
        got = {r: col.count(r) for r in set(col)}
        gaps = got.pop(None, 0)
        assert set(got) == set(s.visits), '%s%s env %d visits %s, the table says %s' % (what, s.name, e, got, sorted(s.visits))
        for r, least in s.visits.items():
            assert got[r] >= least, '%s%s env %d: %d substeps in %s, at least %d wanted' % (what, s.name, e, got[r], r, least)
        assert s.gap or gaps == 0, '%s%s env %d: %d substeps with an undecided count' % (what, s.name, e, gaps)


# ---- a sleeping island inside a dense env -----------------------------------------------------------------------------
# Kilobots 0 .. 63 rest asleep on an 8 x 8 lattice (pitch 0.0325 m: every neighbour pair touches, 2 * 8 * 7 = 112 contacts)
# at (-0.6, 0) and are never commanded; the other 192 are the tail of the pitch-0.010 lattice, 0.4 m to the right.  The
# level sweep of the cooperative solver leaves the 112 contacts out (nsorted < ncon) while the regime is decided from ncon.
SLEEPERS, SLEEPER_CONTACTS = 64, 112
SLEEP_SCENE = SimpleNamespace(name='256-sleeping-island', N=256, capacity=4096, substeps=12, visits={'R3': 1, 'R2': 3, 'R1': 2}, gap=False)


def sleeping_island_start(E):
    N = SLEEP_SCENE.N
    xy, th = scenes.lattice_spawn(E, N, SEED, 0.010, jitter=JITTER)
    xy[:, SLEEPERS:, 0] += 0.4
    i = np.arange(SLEEPERS)
    xy[:, :SLEEPERS, 0] = -0.6 + (i % 8 - 3.5) * 0.0325
    xy[:, :SLEEPERS, 1] = (i // 8 - 3.5) * 0.0325
    sleep_time = np.zeros((E, N), np.float32)
    sleep_time[:, :SLEEPERS] = -1.0
    return xy, th, sleep_time


def sleeping_island_actions(E, k):
    a = actions(E, SLEEP_SCENE.N, k)
    a[:, :SLEEPERS] = 0.0
    return a


def sleeper_entries(ws_cnt):
    """Per env the number of packed warm-start entries owned by kilobots 0 .. 63: the list is packed in ascending owner
    id, so they are its first entries."""
    return np.asarray(ws_cnt)[:, :SLEEPERS].astype(np.int64).sum(axis=1)
