"""Guard bands and poisoned dead state for the kernels' buffers.

The suite compares the kernels with the oracle in memory that hides three kinds of error: a store past a buffer lands in the
allocator's padding, and the memory the contract calls dead -- the tail of the packed warm-start store behind
sum(ws_cnt[e]), kb_buffers.scratch -- is zero or holds last substep's nearly right records.  This module gives the tests

    Arena              one uint8 tensor full of the canary byte; take() hands out views with a canary band on both sides,
                       check() finds the first changed band byte
    guard              moves the bound buffers of a KilobotSim into an arena
    poison_dead_store  makes every dead entry of the store look like a live kilobot partner with a large impulse
    poison_scratch     fills scratch with ones, or with what another scene left there

Every poison word is in range whichever way a kernel reads it (an index below num_bots, a small count, a finite float): a
kernel with the bug computes something else, it does not leave its buffers.  No 0xFF fills, NaNs or huge words in here.

Shared by tests/test_guarded_cpu.py (the arena itself; the store contract on the oracle) and
tests/test_state_isolation_gpu.py (every kernel between bands and over poison, device against device)."""
import numpy as np
import torch

from gym_kilobots_amd import _native as nat

CANARY = 0xA5
ALIGN = 256
MIN_BAND = 4096


def _round_up(n, a):
    return -(-n // a) * a


def band_bytes(row_bytes):
    """Bytes of the band on either side of a view whose env slice has row_bytes: an index that is off by a whole env still
    lands inside the band."""
    return _round_up(max(MIN_BAND, int(row_bytes)), ALIGN)


def footprint(nbytes, row_bytes):
    """Arena bytes that one take() of nbytes uses at the most."""
    return 2 * band_bytes(row_bytes) + _round_up(int(nbytes), ALIGN)


class GuardError(AssertionError):
    pass


class Arena:
    def __init__(self, device, nbytes):
        self.device = torch.device(device)
        self.buf = torch.full((int(nbytes) + ALIGN,), CANARY, dtype=torch.uint8, device=self.device)
        self.start = (-self.buf.data_ptr()) % ALIGN
        self.cursor = self.start            # everything in [start, cursor) outside the views is band
        self.views = []                     # (name, first byte, bytes, band bytes in front, band bytes behind)
        self._is_band = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.device)

    def take(self, shape, dtype, row_bytes, name=None):
        """A contiguous view of this shape, 256-byte aligned, with band_bytes(row_bytes) canary bytes in front of it and at
        least as many behind it."""
        shape = tuple(int(s) for s in (shape if hasattr(shape, '__len__') else (shape,)))
        nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty(0, dtype=dtype).element_size()
        band = band_bytes(row_bytes)
        first = self.cursor + band
        end = self.start + _round_up(first + nbytes + band - self.start, ALIGN)
        if end > self.buf.numel():
            raise ValueError('arena of %d bytes is full: %s needs %d more' % (self.buf.numel(), name, end - self.cursor))
        self._is_band[first:first + nbytes] = False
        self.views.append((name or 'view %d' % len(self.views), first, nbytes, band, end - first - nbytes))
        self.cursor = end
        view = self.buf[first:first + nbytes].view(dtype).view(shape)
        assert view.data_ptr() % ALIGN == 0 and view.is_contiguous()
        return view

    def check(self, what=''):
        """All bands against the canary in one reduction and one read-back; GuardError names the buffer, the side, the byte
        offset of the first changed byte (from the view's first byte in front of it, from its end behind it) and its value."""
        n = self.cursor
        if n == self.start:
            return
        bad = self._is_band[:n] & (self.buf[:n] != CANARY)
        pos = torch.where(bad, torch.arange(n, dtype=torch.int64, device=self.device), n).min()
        val = self.buf[pos.clamp(max=n - 1)]
        pos, val = (int(v) for v in torch.stack((pos, val.to(torch.int64))).cpu())
        if pos == n:
            return
        for name, first, nbytes, front, behind in self.views:
            if first - front <= pos < first:
                side, off = 'before', pos - first
                break
            if first + nbytes <= pos < first + nbytes + behind:
                side, off = 'after', pos - (first + nbytes)
                break
        else:
            name, side, off = 'no buffer', 'before', pos
        raise GuardError('%scanary changed: buffer %s, %s, byte offset %d, value 0x%02x' % (what and what + ': ', name, side, off, val))


def sim_arena_bytes(gsim, extra=0):
    """An arena size that holds every bound buffer of a KilobotSim, plus `extra` bytes for views the test takes itself."""
    E = gsim.num_envs
    total = ALIGN
    for name in nat.BUFFER_FIELDS:
        t = getattr(gsim, name, None)
        if t is not None:
            nbytes = t.numel() * t.element_size()
            total += footprint(nbytes, nbytes // E)
    return total + int(extra)


def guard(gsim, arena):
    """Move every tensor of nat.BUFFER_FIELDS that the sim has into the arena (contents preserved; a band of at least one env
    slice on both sides) and bind the handle to the new addresses."""
    E = gsim.num_envs
    for name in nat.BUFFER_FIELDS:
        t = getattr(gsim, name, None)
        if t is None:
            continue
        v = arena.take(t.shape, t.dtype, t.numel() * t.element_size() // E, name)
        v.copy_(t)
        setattr(gsim, name, v)
    gsim._bind()
    return gsim


def guarded_sim(make, extra=0):
    """(sim, arena): the KilobotSim that make() returns, moved into an arena of its own"""
    gsim = make()
    arena = Arena(gsim.device, sim_arena_bytes(gsim, extra))
    return guard(gsim, arena), arena


# ---- poison ---------------------------------------------------------------------------------------------------------------
def live_entries(ws_cnt, cap):
    """[E] int64: the entries of every env's packed list that mean something, min(sum(ws_cnt[e]), cap)"""
    return ws_cnt.sum(1, dtype=torch.int64).clamp(max=cap)


def live_mask(ws_cnt, cap):
    """[E, cap] bool: position p of env e is a live entry"""
    return torch.arange(cap, device=ws_cnt.device)[None, :] < live_entries(ws_cnt, cap)[:, None]


def poison_store_tensors(ws_cnt, ws_key, ws_acc):
    """The rule of poison_dead_store on three torch tensors (ws_key as int32), on whatever device they live."""
    cap, N = ws_key.shape[1], ws_cnt.shape[1]
    live = live_mask(ws_cnt, cap)
    partner = (torch.arange(cap, device=ws_key.device, dtype=torch.int64) % N).to(ws_key.dtype)[None, :].expand_as(ws_key)
    ws_key.copy_(torch.where(live, ws_key, partner))
    ws_acc.copy_(torch.where(live, ws_acc, torch.ones_like(ws_acc)))


def poison_dead_store(gsim):
    """For every env and every position p >= min(sum(ws_cnt[e]), cap): ws_key = p % N, ws_acc = 1.0f -- a live kilobot partner
    with a large finite impulse, so that a read one entry too far changes the trajectory instead of reproducing the zero
    warm start.  On the device, without a synchronisation."""
    poison_store_tensors(gsim.ws_cnt, gsim.ws_key, gsim.ws_acc)


def poison_oracle_store(osim):
    """The same rule on an OracleSim (numpy arrays), in place."""
    poison_store_tensors(torch.from_numpy(osim.ws_cnt), torch.from_numpy(osim.ws_key.view(np.int32)), torch.from_numpy(osim.ws_acc))


def record_stale_scratch(gsim):
    """Keep the bytes the handle's scratch holds now -- after a launch of the twin scene -- for poison_scratch(gsim, 'stale')."""
    gsim._stale_scratch = gsim.scratch.clone()


def poison_scratch(gsim, how):
    """'ones': every 32-bit word of scratch is 1 -- a valid kilobot index for N >= 2, a small count and a finite float.
    'stale': the bytes record_stale_scratch kept: what the same handle's scratch held after a launch of the twin scene (the
    same configuration with another spawn seed), so every index in it is in range for this configuration."""
    if how == 'ones':
        gsim.scratch.view(torch.int32).fill_(1)
    elif how == 'stale':
        gsim.scratch.copy_(gsim._stale_scratch)
    else:
        raise ValueError("how must be 'ones' or 'stale'")


# ---- comparisons, device against device -----------------------------------------------------------------------------------
def bits(t):
    """a float tensor as its bit patterns (torch.equal would call -0.0 and +0.0 equal and a NaN different from itself)"""
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def bound_fields(sim):
    return [n for n in nat.BUFFER_FIELDS if getattr(sim, n, None) is not None]


STORE_LISTS = ('ws_key', 'ws_acc')


def assert_fields_equal(psim, gsim, what, envs=None, skip=()):
    """Every bound field except scratch bit for bit, of ws_key and ws_acc the live entries only; envs: these envs only."""
    names = bound_fields(psim)
    assert names == bound_fields(gsim), what
    sel = slice(None) if envs is None else torch.as_tensor(list(envs), device=psim.ws_cnt.device)
    for name in names:
        if name == 'scratch' or name in STORE_LISTS or name in skip:
            continue
        a, b = bits(getattr(psim, name))[sel], bits(getattr(gsim, name))[sel]
        if not torch.equal(a, b):
            raise AssertionError('%s: field %s differs in %d of %d elements' % (what, name, int((a != b).sum()), a.numel()))
    cap = psim.ws_key.shape[1]
    live = live_mask(psim.ws_cnt, cap)[sel]
    for name in STORE_LISTS:
        a, b = bits(getattr(psim, name))[sel], bits(getattr(gsim, name))[sel]
        zero = torch.zeros_like(a)
        if not torch.equal(torch.where(live, a, zero), torch.where(live, b, zero)):
            raise AssertionError('%s: the live entries of %s differ in %d places' % (what, name, int((live & (a != b)).sum())))
