"""The staging limits that only the device step has, restated on the CPU: for one substep of every env, the quantities the
step kernels count into packed counters, 8-bit ranks and fixed LDS arrays, and the largest value of each that must still be
bit-exact against the oracle.  No GPU is needed.

What is counted (`evaluate`; per env and substep):

    partners    [N, 5]: per kilobot and direction k = 0 .. 4 (same cell, E, N, NE, NW -- the cell of the partner as seen from
                the owner of the contact, oracle/kb_oracle.c CLS_*) the kilobot-kilobot contacts it owns
    groups      {(class, cell of the owner): contacts}: the rank of a contact counts inside such a group, the largest rank of a
                group is its size - 1
    fixtures    [num_fixtures]: kilobots that touch the fixture
    depth       the deepest dependency level of the env (tools/placement_model.py: islands_and_depths); None with objects or
                mixed drive laws, whose kernels have no level table
    candidates  kilobots that the continuous step must take through its event loop: awake, and tests/toi_scenes.py: no_event
                fails on some wall between the start pose and the pose behind b2Island::Solve
    hidden      the side oracle itself ran out of slots or capacity (a kilobot with more than 64 contacts): the counts are
                lower bounds, and what they do not exceed proves nothing
    ncon        contacts of the substep, and max_island, the contacts of its largest island (walls included): they decide the
                solver path (tests/solver_regimes.py; `level_sweep`)

The contacts are read from a SIDE oracle: a copy of the state at the start of the substep, stepped once with ws_slots = 64,
contact_capacity = 65528 and toi_walls = 0.  The first two keep a small ws_slots or capacity of the scene from hiding
contacts from the model (the solve itself does not depend on either: a contact beyond the slots of its owner is solved, only
never stored); the third leaves the poses as the kernel holds them when it collects the candidates.

What the limits are (`limits`; from the handle -- kb_lds_staging_entries, kb_block_threads, num_bots -- and the formulas of
include/kilobots_hip.h, not from the kernel source).  Each is the largest value that is still exact:

    partners    63 per kilobot and direction (a 6-bit field of a packed counter; the 64th partner is flagged)
    rank        255 (8 bits: a group of 256 contacts is exact, the 257th contact is flagged)
    fixture     64 kilobots on one fixture (kernels with objects or mixed laws)
    depth       44 x waves - 2 levels, where the cooperative level sweep runs: kernels without objects, workgroups of two waves
                or more (a one-wave workgroup keeps the list sweep and has no level table to overflow)
    candidates  min(staging entries, num_bots) without objects, staging entries // 2 with objects or mixed laws

`exceeded` names the limits a substep is over.  The partner limit cannot be the only one: the partners of one kilobot in one
direction lie in ONE cell, inside the half disc of one diameter around the owner.  Three sectors of 60 degrees cover that half
disc and each has diameter one kilobot diameter, so the kilobots of a sector all touch each other: 64 partners give at least
22 + 21 + 21 in the sectors and 231 + 210 + 210 = 651 same-cell contacts in the partner cell, 63 partners 3 x 210 = 630 -- the
group (CLS_SAME, that cell) is past rank 255 long before (the same-cell direction: six sectors, 63 own contacts + 300).  The
partner guard is therefore never the first to fire, and no scene can sit AT 63 partners with a clean status;
tests/test_limits_cpu.py holds the model to that on piles.

The model is the reference for the FLAGS; the oracle stays the reference for the bits."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

from oracle import oracle as O
from tests import toi_scenes as TS
from tools import placement_model as PM

f32 = np.float32
CELL_SIZE, MAX_CELLS = 0.875, 8192          # kb_common.h (world units; the cell doubles until it holds a kilobot diameter and the grid fits)
KEY_WALL, KEY_OBJ = 0x10000, 0x20000        # oracle/kb_oracle.c: keys of the packed list
SIDE_SLOTS, SIDE_CAPACITY = 64, 65528
PARTNERS, RANK, FIXTURE = 63, 255, 64
LEVELS_PER_WAVE = 44
DIR_OF_CLASS = {0: 0, 1: 1, 2: 1, 3: 2, 4: 2, 5: 3, 6: 3, 7: 4, 8: 4}      # CLS_SAME, CLS_E (+ parity), CLS_N, CLS_NE, CLS_NW -> k
BIT_STAGING, BIT_CANDIDATES = 4, 8


def grid(cfg):
    """(xmin, ymin, xmax, ymax, inv_cell, gw, gh) in float32 world units, as kb_create derives them"""
    W, H = f32(cfg.world_width) * f32(25.0), f32(cfg.world_height) * f32(25.0)
    cell = f32(CELL_SIZE)
    while cell < f32(2.0) * f32(cfg.bot_radius) * f32(25.0):
        cell = cell * f32(2.0)
    while True:
        inv = f32(1.0) / cell
        gw, gh = max(int(np.ceil(W * inv)), 1), max(int(np.ceil(H * inv)), 1)
        if gw * gh <= MAX_CELLS:
            break
        cell = cell * f32(2.0)
    return f32(-0.5) * W, f32(-0.5) * H, f32(0.5) * W, f32(0.5) * H, inv, gw, gh


def cells(cfg, x, y):
    xmin, ymin, _, _, inv, gw, gh = grid(cfg)
    cx = np.clip(np.floor((np.asarray(x, f32) - xmin) * inv).astype(np.int64), 0, gw - 1)
    cy = np.clip(np.floor((np.asarray(y, f32) - ymin) * inv).astype(np.int64), 0, gh - 1)
    return cx, cy, gw


def side_oracle(osim, **changes):
    """A copy of an OracleSim's whole state under a changed configuration (the packed store is repacked to the new capacity)"""
    cfg = O.Config.from_buffer_copy(osim.cfg)
    for k, v in changes.items():
        setattr(cfg, k, v)
    side = O.OracleSim(cfg)
    for name, _ in O.State._fields_:
        src = getattr(osim, name, None)
        if src is None or name in ('ws_key', 'ws_acc', 'status'):
            continue
        getattr(side, name)[...] = src
    live = np.minimum(osim.ws_cnt.astype(np.int64).sum(1), osim.cap)
    assert (live <= side.cap).all()
    for e, n in enumerate(live):
        side.ws_key[e, :n] = osim.ws_key[e, :n]
        side.ws_acc[e, :n] = osim.ws_acc[e, :n]
    return side


def env_contacts(cfg, x, y, ws_key, ws_cnt):
    """[(class, group, A, B)] of the kilobot-kilobot and wall contacts in canonical order (A < 0: wall -1 - A), and
    [(owner, fixture)] of the kilobot-fixture contacts; tools/placement_model.py: env_contacts for any arena"""
    N = len(ws_cnt)
    cx, cy, gw = cells(cfg, x, y)
    owner = np.repeat(np.arange(N), np.asarray(ws_cnt).astype(np.int64))
    rows, touches = [], []
    for a, k in zip(owner.tolist(), np.asarray(ws_key)[:len(owner)].astype(np.int64).tolist()):
        if k >= KEY_OBJ:
            touches.append((a, k - KEY_OBJ))
        elif k >= KEY_WALL:
            rows.append((PM.CLS_WALL, a, -1 - (k - KEY_WALL), a))
        else:
            d = (int(cx[k] - cx[a]), int(cy[k] - cy[a]))
            cls = PM.DIRS[d]
            if d[0] != 0:
                cls += int(cx[a]) & 1
            elif d[1] != 0:
                cls += int(cy[a]) & 1
            rows.append((cls, int(cy[a]) * gw + int(cx[a]), a, k))
    rows.sort()
    return rows, touches


def _ranked(rows):
    out, rank, prev = [], 0, None
    for cls, grp, a, b in rows:
        rank = rank + 1 if (cls, grp) == prev else 0
        prev = (cls, grp)
        out.append((cls, rank, a, b))
    return out


def no_event_all_walls(cfg, x0, y0, x1, y1):
    """[N] bool: kb_toi_no_event holds on all four walls (tests/toi_scenes.py: sweep_dists, no_event, in any arena)"""
    xmin, ymin, xmax, ymax = grid(cfg)[:4]
    _, tt = TS.thresholds(cfg.bot_radius)

    def dists(x, y):
        return np.stack([x - xmin, y - ymin, xmax - x, ymax - y])
    with np.errstate(invalid='ignore'):
        xa, ya = TS._lerp(0.0, x0, x1), TS._lerp(0.0, y0, y1)
        xb, yb = TS._lerp(1.0, x0, x1), TS._lerp(1.0, y0, y1)
    return TS.no_event(dists(xa, ya), dists(xb, yb), tt).all(0)


def evaluate(osim, light_action=None, flags=0):
    """The counted quantities of the substep that `osim` is about to take, one SimpleNamespace per env.  osim is not changed."""
    cfg = osim.cfg
    E, N = cfg.num_envs, cfg.num_bots
    side = side_oracle(osim, ws_slots=SIDE_SLOTS, contact_capacity=SIDE_CAPACITY, toi_walls=0)
    x0, y0 = osim.x.copy(), osim.y.copy()
    side.step(1, light_action=light_action, flags=flags)
    F = (cfg.num_fixtures or cfg.num_objects) if cfg.num_objects > 0 else 0      # (num_fixtures 0: one fixture per object)
    plain = cfg.num_objects == 0 and cfg.drive_mode != O.DRIVE_MIXED
    out = []
    for e in range(E):
        rows, touches = env_contacts(cfg, x0[e], y0[e], side.ws_key[e], side.ws_cnt[e])
        partners = np.zeros((N, 5), np.int64)
        groups = {}
        for cls, grp, a, b in rows:
            if cls == PM.CLS_WALL:
                continue
            partners[a, DIR_OF_CLASS[cls]] += 1
            groups[(cls, grp)] = groups.get((cls, grp), 0) + 1
        fixtures = np.zeros(max(F, 1), np.int64)
        for a, f in touches:
            fixtures[f] += 1
        depth = island = None
        if plain:
            roots, lv = PM.islands_and_depths(_ranked(rows), N)
            depth = max(lv) if lv else 0
            island = int(np.bincount(roots).max()) if roots else 0
        awake = side.sleep_time[e] >= 0.0 if cfg.allow_sleep else np.ones(N, bool)
        cand = awake & ~no_event_all_walls(cfg, x0[e], y0[e], side.x[e], side.y[e]) & bool(cfg.toi_walls)
        out.append(SimpleNamespace(partners=partners, groups=groups, fixtures=fixtures[:F], depth=depth, candidates=int(cand.sum()),
                                   candidate_ids=np.flatnonzero(cand), ncon=len(rows) + len(touches), max_island=island,
                                   asleep=int((~awake).sum()), hidden=bool(side.status[e] & 3),
                                   max_partners=int(partners.max()) if N else 0, max_rank=max(groups.values(), default=0) - 1,
                                   max_fixture=int(fixtures.max())))
    return out


def limits(num_bots, staging_entries, block_threads, plain):
    """The largest exact value of every counted quantity.  plain: a kernel without objects and without mixed drive laws.
    depth is None where no level table exists (kernels with objects or mixed laws; one-wave workgroups)."""
    nw = block_threads // 64
    return SimpleNamespace(partners=PARTNERS, rank=RANK, fixture=FIXTURE,
                           depth=LEVELS_PER_WAVE * nw - 2 if plain and nw > 1 else None,
                           candidates=min(staging_entries, num_bots) if plain else staging_entries // 2)


def handle_limits(lib, nat, cfg_kw, num_bots, drive_mode=O.DRIVE_VELOCITY, light_type=O.LIGHT_NONE, block_threads=0):
    """(limits, SimpleNamespace(threads, staging, capacity, variant)) of the handle kb_create makes -- no GPU needed"""
    cfg = nat.default_config(1, num_bots, drive_mode, light_type, **cfg_kw)
    h = C.c_void_p()
    rc = lib.kb_create(C.byref(cfg), C.byref(h))
    assert rc == nat.KB_OK, rc
    try:
        if block_threads:
            rc = lib.kb_set_block_threads(h, block_threads)
            assert rc == nat.KB_OK, rc
        shape = SimpleNamespace(threads=lib.kb_block_threads(h), staging=lib.kb_lds_staging_entries(h),
                                capacity=lib.kb_contact_capacity(h), variant=lib.kb_variant_index(h))
    finally:
        lib.kb_destroy(h)
    plain = cfg.num_objects == 0 and drive_mode != O.DRIVE_MIXED
    return limits(num_bots, shape.staging, shape.threads, plain), shape


GIANT_ISLAND, REG_CONTACTS = 256, 128        # kb_common.h; tests/solver_regimes.py


def level_sweep(q, lim, shape, solver_mode):
    """Does the cooperative level sweep -- the only path with a level table -- run env-substep q?  True / False / None (the
    counts do not decide it).  It runs in kernels without objects on workgroups of two waves or more: always under
    solver_mode 2 and 4 and for an island of more than GIANT_ISLAND contacts; under solver_mode 0 whenever the register
    solver cannot take the env -- more contacts than the staging area holds, or a wave with more than 128.  With kilobots
    asleep the answer is None: the contacts of a sleeping island are in no level, and the model's depth counts them."""
    if lim.depth is None:
        return False
    if q.asleep:
        return None
    nw = shape.threads // 64
    if solver_mode in (2, 4) or q.max_island > GIANT_ISLAND:
        return True
    if solver_mode != 0 or q.ncon <= REG_CONTACTS:
        return False
    if q.ncon > min(shape.staging, shape.capacity) or q.ncon > REG_CONTACTS * nw:
        return True
    return None


def exceeded(q, lim, sweep=None):
    """The limits env-substep q is over: a set of 'partners', 'rank', 'fixture', 'depth', 'candidates'.
    sweep: does the cooperative level sweep run this substep?  True / False / None (not decided by the contact count:
    tests/solver_regimes.py); with None a depth past the limit is reported as 'depth?' -- the device may flag it or not."""
    over = set()
    if q.max_partners > lim.partners:
        over.add('partners')
    if q.max_rank > lim.rank:
        over.add('rank')
    if len(q.fixtures) and q.max_fixture > lim.fixture:
        over.add('fixture')
    if lim.depth is not None and q.depth is not None and q.depth > lim.depth and sweep is not False:
        over.add('depth' if sweep else 'depth?')
    if q.candidates > lim.candidates:
        over.add('candidates')
    return over


def expected_bits(over):
    """status bits 2 and 3 that the device must raise for a set from `exceeded` ('depth?' asks for nothing)"""
    return (BIT_STAGING if over & {'partners', 'rank', 'fixture', 'depth'} else 0) | (BIT_CANDIDATES if 'candidates' in over else 0)
