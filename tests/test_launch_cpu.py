"""The launch shape of a handle (gym_kilobots_amd/csrc/kb_launch.h: plan_launch), checked without a GPU against
tests/golden/launch_plan.txt, which records what kb_create and kb_set_block_threads derived before the derivation moved
into that header: workgroup size, contact capacity, LDS staging entries, cell heads, LDS image and offsets, register tier
and instantiation, or the error code of a refused configuration.  The header is plain C++ and is compiled here with the
system compiler; the library is checked through its ABI on the same rows."""
import ctypes as C
import os
import subprocess

import pytest

from gym_kilobots_amd import _native as nat
from gym_kilobots_amd import build as kb_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <cstdio>
#include "kb_launch.h"
using namespace kb;
int main() {
    int v[11];
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8], &v[9], &v[10]) == 11) {
        const Plan p = plan_launch({v[0], v[1], v[2], v[3] != 0, v[4], v[5], v[6] != 0, v[7] != 0, v[8], v[9], v[10]});
        if (p.status != KB_OK) { printf("%d\n", p.status); continue; }
        const Variant &k = p.variant;
        printf("%d %d %d %d %d %d %d %d %d %d : %d %d %d %d %d %d %d %d\n", p.status, p.cap, p.capL, p.nhead, p.hmask, p.threads,
               p.lds_total, p.islmin_off, p.botlaw_off, p.tier, k.drive, k.light, k.obj, k.fn, k.tier, k.poly, k.sense, k.sleep);
    }
    return 0;
}
'''

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
    src = tmp_path / 'launch.cpp'
    src.write_text(PROGRAM)
    exe = str(tmp_path / 'launch')
    subprocess.check_call(['g++', '-std=c++17', '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'gym_kilobots_amd', 'csrc'),
                           str(src), '-o', exe])
    stdin = '\n'.join(' '.join(map(str, inputs)) for inputs, _ in rows).encode()
    out = subprocess.run([exe], input=stdin, stdout=subprocess.PIPE, check=True).stdout.decode().split('\n')
    assert len(out) >= len(rows)
    for (inputs, want), got in zip(rows, out):
        assert got == want, 'plan input %s: %s, recorded %s' % (inputs, got, want)


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


@pytest.fixture(scope='module')
def lib():
    kb_build.build()
    return nat.load()


def test_library_matches_the_recorded_shapes(lib):
    h = C.c_void_p()
    for inputs, want in golden_rows():
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
        lib.kb_destroy(h)
