"""kb_sense_neighbors without a GPU: the symbol is exported and bound, the host-side validation answers in the order the
header gives (arguments before the bound check, so none of it needs a device), and the kernels keep their k best
candidates in registers (no scratch, no spills in the code object's metadata)."""
import ctypes as C
import os
import re


from gym_kilobots_amd import _native as nat
from tests.host_common import handle, lib  # noqa: F401
from tests.sensing_common import kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, 'include', 'kilobots_hip.h')).read()
    assert re.search(r'\bint\s+kb_sense_neighbors\s*\(', hdr)
    m = re.search(r'#define\s+KB_MAX_NEIGHBORS\s+(\d+)', hdr)
    assert m and int(m.group(1)) == nat.MAX_NEIGHBORS == 16
    assert 'kb_sense_neighbors' in nat.EXPORTS
    assert hasattr(lib, 'kb_sense_neighbors')
    assert lib.kb_sense_neighbors.argtypes is not None and len(lib.kb_sense_neighbors.argtypes) == 7


def test_validation_on_an_unbound_handle(lib, handle):
    """Nothing here launches: the pointers are never dereferenced on the host (any non-NULL value will do)."""
    idx, rel, cnt = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)
    bad = [
        ('k = 0', (handle, 0.07, 0, idx, rel, cnt, None)),
        ('k = 17', (handle, 0.07, 17, idx, rel, cnt, None)),
        ('radius = 0', (handle, 0.0, 8, idx, rel, cnt, None)),
        ('radius = -1', (handle, -1.0, 8, idx, rel, cnt, None)),
        ('radius = NaN', (handle, float('nan'), 8, idx, rel, cnt, None)),
        ('NULL d_index', (handle, 0.07, 8, None, rel, cnt, None)),
        ('NULL d_rel', (handle, 0.07, 8, idx, None, cnt, None)),
        ('NULL sim', (None, 0.07, 8, idx, rel, cnt, None)),
    ]
    for what, args in bad:
        lib.kb_sense_neighbors(None, 0.07, 8, idx, rel, cnt, None)     # (leaves a message that the next call must replace)
        assert lib.kb_sense_neighbors(*args) == nat.KB_EINVAL, what
        msg = lib.kb_last_error()
        assert msg and b'kb_sense_neighbors' in msg, what
    for k in (1, 8, 16):
        for c in (cnt, None):       # d_count is optional
            assert lib.kb_sense_neighbors(handle, 0.07, k, idx, rel, c, None) == nat.KB_ENOTBOUND
            assert b'kb_sense_neighbors' in lib.kb_last_error() and b'kb_bind' in lib.kb_last_error()


def test_argument_errors_come_before_the_bound_check(lib, handle):
    """k, radius and NULL outputs are reported as KB_EINVAL although the handle is unbound as well."""
    idx, rel = C.c_void_p(0x1000), C.c_void_p(0x2000)
    assert lib.kb_sense_neighbors(handle, 0.07, 17, idx, rel, None, None) == nat.KB_EINVAL
    assert lib.kb_sense_neighbors(handle, float('nan'), 4, idx, rel, None, None) == nat.KB_EINVAL
    assert lib.kb_sense_neighbors(handle, 0.07, 4, idx, rel, None, None) == nat.KB_ENOTBOUND


def test_kernels_use_no_scratch_and_spill_nothing(lib):
    """The k best (d2, j) keys live in registers: every instantiation of the list kernel has a zero private segment and zero
    spill counts in the metadata of the code object that was linked (the assembly build() keeps next to the object)."""
    seen = 0
    for name, fields in kernel_metadata('kb_neighbors_kernel'):
        seen += 1
        for key in ('.private_segment_fixed_size', '.sgpr_spill_count', '.vgpr_spill_count'):
            assert fields[key] == 0, (name, key, fields[key])
    assert seen == 3, 'expected the instantiations for 4, 8 and 16 slots, found %d' % seen
