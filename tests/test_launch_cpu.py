"""The launch shape of a handle (gym_kilobots_amd/csrc/kb_launch.h: plan_launch), checked without a GPU against
tests/golden/launch_plan.txt, which records what kb_create and kb_set_block_threads derived before the derivation moved
into that header: workgroup size, contact capacity, LDS staging entries, cell heads, LDS image and offsets, register tier
and instantiation, or the error code of a refused configuration.  The header is plain C++ and is compiled here with the
system compiler; the library is checked through its ABI on the same rows."""
import ctypes as C
import os
import subprocess


from gym_kilobots_amd import _native as nat
from tests.host_common import lib, plan_rows  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the arenas of the golden grid by their cell count (2 x 1.5 m: 58 x 43 cells of 0.875 world units, 0.6 x 0.6 m: 18 x 18)
ARENAS = {2494: (2.0, 1.5), 324: (0.6, 0.6)}


def golden_rows():
    rows = []
    for line in open(os.path.join(ROOT, 'tests', 'golden', 'launch_plan.txt')):
        if line.startswith('#'):
            continue
        inputs, result = line.split(':', 1)
        rows.append(([int(x) for x in inputs.split()], ' '.join(result.split())))
    return rows


def test_plan_matches_the_recorded_shapes(tmp_path):
    rows = golden_rows()
    for (inputs, want), (got, index) in zip(rows, plan_rows(tmp_path, rows)):
        assert got == want, 'plan input %s: %s, recorded %s' % (inputs, got, want)
        # every recorded instantiation is one of the library's list
        assert index is None or 0 <= index < 176, inputs


def config(inputs):
    N, M, F, discs, drive, light, sense, sleep, ncell, capacity, _ = inputs
    w, h = ARENAS[ncell]
    cfg = nat.default_config(1, N, drive, light, world_width=w, world_height=h, contact_capacity=capacity, allow_sleep=sleep,
                             sense_radius=0.07 if sense else 0.0)
    # the shapes only count through the fixture count and "all discs"
    cfg.num_objects = M
    cfg.num_fixtures = F if F != M else 0
    for f in range(F):
        cfg.obj_fixture_body[f] = f * M // F
        cfg.obj_shape[f] = nat.SHAPE_CIRCLE if discs else nat.SHAPE_BOX
        cfg.obj_radius[f] = 0.05
        cfg.obj_verts[f][0][0], cfg.obj_verts[f][0][1] = 0.05, 0.03
    return cfg


def test_library_matches_the_recorded_shapes(lib, tmp_path):
    h = C.c_void_p()
    rows = golden_rows()
    accepted = 0
    for (inputs, want), (_, index) in zip(rows, plan_rows(tmp_path, rows)):
        threads = inputs[-1]
        cfg = config(inputs)
        rc = lib.kb_create(C.byref(cfg), C.byref(h))
        if threads == 0 and rc != nat.KB_OK:
            assert str(rc) == want, inputs
            continue
        assert rc == nat.KB_OK, inputs
        if threads:
            rc = lib.kb_set_block_threads(h, threads)
        fields = want.split()
        if rc != nat.KB_OK:
            assert fields == [str(rc)], inputs
        else:
            status, cap, capL, _, _, wg, lds = (int(x) for x in fields[:7])
            assert (rc, lib.kb_contact_capacity(h), lib.kb_lds_staging_entries(h), lib.kb_block_threads(h), lib.kb_lds_bytes(h)) == \
                (status, cap, capL, wg, lds), inputs
            # ... and runs the instantiation that the header selects for the row (kb_variant_index follows kb_set_block_threads)
            assert index is not None and lib.kb_variant_index(h) == index, inputs
            accepted += 1
        lib.kb_destroy(h)
    assert accepted > 0


ALIGNMENT_PROGRAM = r'''
#include <cstdio>
#include "kb_launch.h"
using namespace kb;
int main() {
    int bad = 0;
    for (int mixed = 0; mixed < 2; ++mixed)
        for (int M = mixed ? 0 : 1; M <= KB_MAX_OBJECTS; ++M)
            for (int N = 1; N <= 1024; ++N) {
                const Plan p = plan_launch({N, M, M, false, mixed ? KB_DRIVE_MIXED : KB_DRIVE_VELOCITY, 0, true, true, 2494, 0, 0});
                if (p.status != KB_OK) continue;
                const int NP = (N + 3) & ~3, NB = NP + KB_MAX_OBJECTS + 4, fx = lds::fixed(true, p.threads / 64);
                for (int k = 0; k < lds::BOT16_COUNT; ++k)
                    if (lds::bot16(fx, NB, p.capL, NP, k) % 4 != 0 && ++bad <= 5) printf("N %d M %d capL %d array %d at %d\n", N, M, p.capL, k, lds::bot16(fx, NB, p.capL, NP, k));
                if (lds::head(fx, NB, p.capL, NP) % 4 != 0 && ++bad <= 5) printf("N %d M %d capL %d head\n", N, M, p.capL);
            }
    printf("%d\n", bad);
    return 0;
}
'''


def test_word_atomics_on_the_16_bit_arrays_are_aligned(tmp_path):
    """The kernels with objects (and mixed laws) run 32-bit LDS atomics on 16-bit arrays: two neighbour counters per word in
    newOff (fused sensing), compare-and-swap on the cell heads.  An odd number of staging entries (3 N + 64 of an odd swarm,
    e.g. 129 kilobots with two objects: 451) once left newOff at a half-word offset, and the sensing pass faulted."""
    src = tmp_path / 'align.cpp'
    src.write_text(ALIGNMENT_PROGRAM)
    exe = str(tmp_path / 'align')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'gym_kilobots_amd', 'csrc'),
                           str(src), '-o', exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, check=True).stdout.decode().strip().split('\n')
    assert out[-1] == '0', 'misaligned: ' + '; '.join(out[:-1])
