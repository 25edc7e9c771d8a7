"""What the tests of the C ABI and of the host-side headers share, none of which needs a GPU: the loaded library as a
fixture, a handle without buffers, the prototypes of include/kilobots_hip.h against ctypes signatures, and plan_launch of
gym_kilobots_amd/csrc/kb_launch.h compiled with the system compiler.

A test module brings a fixture in by name (`from tests.host_common import lib  # noqa: F401`): pytest finds a fixture in
the namespace of the module that uses it, and a module-scoped one is made once per such module."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from gym_kilobots_amd import _native as nat
from gym_kilobots_amd import build as kb_build
from tests import geometry_scenes as GS
from tests import objects_ref
from tests import solver_regimes as SR
from tests import variant_census as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- fixtures --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    kb_build.build()
    return nat.load()


@pytest.fixture()
def handle(lib):
    h = C.c_void_p()
    cfg = nat.default_config(4, 64)
    assert lib.kb_create(C.byref(cfg), C.byref(h)) == 0, lib.kb_last_error()
    yield h
    lib.kb_destroy(h)


@pytest.fixture(scope='module')
def tab(lib):
    with Handle(lib) as h:
        return objects_ref.tables(nat.outline(h))


@pytest.fixture(scope='module')
def variants(tmp_path_factory):
    """kb_variants as tuples (drive, light, obj, fn, tier, poly, sense, sleep), from the header compiled on the host"""
    listed, _ = VC.host_census(tmp_path_factory.mktemp('plan'), [SR.plan_inputs(64, 0, 0)])
    return listed


def word_bits(a):
    """The 32-bit words of a numpy array as they are: demands a 4-byte dtype and converts nothing (objects_ref.bits converts
    to float32 first)."""
    return np.ascontiguousarray(a).view(np.uint32)


class Handle(object):
    """A kb_sim without buffers: what kb_get_outline and the host-side validation of an entry point need."""

    def __init__(self, lib, E=4, N=64, **kw):
        self.lib, self.h = lib, C.c_void_p()
        cfg = nat.default_config(E, N, **kw)
        rc = lib.kb_create(C.byref(cfg), C.byref(self.h))
        assert rc == 0, lib.kb_last_error()

    def __enter__(self):
        return self.h

    def __exit__(self, *exc):
        self.lib.kb_destroy(self.h)


# ---- the header's prototypes against ctypes ----------------------------------------------------------------------------------
SCALARS = {'int': C.c_int, 'float': C.c_float, 'int64_t': C.c_int64, 'uint32_t': C.c_uint32, 'size_t': C.c_size_t}
MIRRORS = {'kb_config': nat.KbConfig, 'kb_buffers': nat.KbBuffers, 'kb_outline': nat.KbOutline, 'kb_render_style': nat.KbRenderStyle,
           'kb_reset_params': nat.KbResetParams, 'kb_episode_init': nat.KbEpisodeInit}


def ctypes_of(c_type, returned=False):
    """The ctypes types that may stand for a C type of the header (qualifiers and the parameter's name taken off)."""
    base, stars = c_type.replace('*', ' ').split(), c_type.count('*')
    base = ' '.join(w for w in base if w != 'const')
    if stars == 0:
        return (None,) if base == 'void' and returned else (SCALARS[base],)
    if returned and (base, stars) == ('char', 1):
        return (C.c_char_p,)
    if stars == 1 and base in MIRRORS:
        return (C.c_void_p, C.POINTER(MIRRORS[base]))
    return (C.c_void_p,)


@functools.lru_cache(None)
def prototypes():
    """{name: (return type, [parameter types])} as C text, of every function include/kilobots_hip.h declares."""
    hdr = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', 'kilobots_hip.h')).read(), flags=re.S)
    found = {}
    for ret, name, params in re.findall(r'^([\w \*]+?)\s*\b(kb_[a-z_]+)\s*\(([^()]*)\)\s*;', hdr, flags=re.M):
        params = [] if params.strip() == 'void' else [re.sub(r'\w+\s*$', '', p.strip()) for p in params.split(',')]
        assert name not in found and all(p.strip() for p in params), name
        found[name] = (ret, params)
    return found


def abi_mismatches(signatures, bound):
    """Where `signatures` (a table like nat.SIGNATURES) or what `bound(name)` returns as (restype, argtypes) departs from
    the header's prototypes: one line per return type or parameter."""
    protos, bad = prototypes(), []
    if set(protos) != set(signatures):
        bad.append('names: %s' % sorted(set(protos) ^ set(signatures)))
    for name, (ret, params) in protos.items():
        for what, (restype, argtypes) in (('table', signatures.get(name, (0, []))), ('library', bound(name))):
            if restype not in ctypes_of(ret, returned=True):
                bad.append('%s: %s returns %r for %r' % (what, name, restype, ret))
            if len(argtypes or []) != len(params):
                bad.append('%s: %s takes %d arguments for %d' % (what, name, len(argtypes or []), len(params)))
            bad += ['%s: %s argument %d is %r for %r' % (what, name, k, a, p) for k, (a, p) in enumerate(zip(argtypes or [], params))
                    if a not in ctypes_of(p)]
    return bad


# ---- plan_launch on the host -------------------------------------------------------------------------------------------------
def compile_host(tmp_path, name, program, include=None):
    src = tmp_path / (name + '.cpp')
    src.write_text(program)
    exe = str(tmp_path / name)
    include = include or os.path.join(ROOT, 'gym_kilobots_amd', 'csrc')
    subprocess.check_call(['g++', '-std=c++17', '-O2', '-I', os.path.join(ROOT, 'include'), '-I', include, str(src), '-o', exe])
    return exe


PLAN_PROGRAM = r'''
#include <cstdio>
#include "kb_launch.h"
using namespace kb;
int main() {
    int v[11];
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8], &v[9], &v[10]) == 11) {
        const Plan p = plan_launch({v[0], v[1], v[2], v[3] != 0, v[4], v[5], v[6] != 0, v[7] != 0, v[8], v[9], v[10]});
        if (p.status != KB_OK) { printf("%d\n", p.status); continue; }
        const Variant &k = p.variant;
        printf("%d %d %d %d %d %d %d %d %d %d : %d %d %d %d %d %d %d %d # %d\n", p.status, p.cap, p.capL, p.nhead, p.hmask, p.threads,
               p.lds_total, p.islmin_off, p.botlaw_off, p.tier, k.drive, k.light, k.obj, k.fn, k.tier, k.poly, k.sense, k.sleep,
               variant_index(p.variant));
    }
    return 0;
}
'''


def plan_rows(tmp_path, rows):
    """plan_launch of the header on the inputs of `rows`: [(result in the format of tests/golden/launch_plan.txt, position of
    the instantiation in kb_variants or None for a refused configuration)]"""
    src = tmp_path / 'launch.cpp'
    src.write_text(PLAN_PROGRAM)
    exe = str(tmp_path / 'launch')
    subprocess.check_call(['g++', '-std=c++17', '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'gym_kilobots_amd', 'csrc'),
                           str(src), '-o', exe])
    stdin = '\n'.join(' '.join(map(str, inputs)) for inputs, _ in rows).encode()
    out = subprocess.run([exe], input=stdin, stdout=subprocess.PIPE, check=True).stdout.decode().split('\n')
    assert len(out) >= len(rows), 'plan_launch printed %d lines for %d rows' % (len(out), len(rows))
    plans = []
    for line in out[:len(rows)]:
        result, _, index = line.partition(' # ')
        plans.append((result, int(index) if index else None))
    return plans


# per input row of stdin (the columns of tests/golden/launch_plan.txt): the status of plan_launch, where islMin lies
# (1 over the bin boundaries, 2 over the staged pairs, 3 behind the image, 0 not a sorted-bin kernel, -1 none of these)
# and whether the NB words at the place the kernel takes end inside the image
BRANCH_PROGRAM = r'''
#include <cstdio>
#include "kb_launch.h"
using namespace kb;
int main() {
    int v[11];
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8], &v[9], &v[10]) == 11) {
        const Plan p = plan_launch({v[0], v[1], v[2], v[3] != 0, v[4], v[5], v[6] != 0, v[7] != 0, v[8], v[9], v[10]});
        const int NP = (v[0] + 3) & ~3, NB = NP + KB_MAX_OBJECTS + 4;
        int branch = 0, inside = 1;
        if (p.status == KB_OK && v[1] == 0 && v[4] != KB_DRIVE_MIXED) {
            const bool hashed = p.hmask != 0;
            branch = p.islmin_off == ldsb::binE(NB, NP, hashed, p.capL) ? 1 : p.islmin_off == ldsb::con32(NB, NP, hashed, p.capL, 0) ? 2
                   : p.islmin_off == ldsb::total(NB, NP, hashed, p.capL, p.nhead, p.threads / 64) ? 3 : -1;
            const int at = p.variant.fn ? ldsb::binE(NB, NP, false, p.capL) : p.islmin_off;
            inside = !v[7] || at + 4 * NB <= p.lds_total;
        }
        printf("%d %d %d\n", p.status, branch, inside);
    }
    return 0;
}
'''


def plans_of(tmp, rows, threads=None):
    """plan_launch of the header for rows of either table of tests/geometry_scenes.py, at kb_create's width or at threads[i]
    (0: kb_create's): [(row, fields of the plan as ints, template arguments of the instantiation, its index, islMin branch, inside)]"""
    inputs = [(GS.plan_inputs(g, threads[i] if threads else 0), '') for i, g in enumerate(rows)]
    plans = plan_rows(tmp, inputs)
    exe = compile_host(tmp, 'branch', BRANCH_PROGRAM)
    stdin = '\n'.join(' '.join(map(str, v)) for v, _ in inputs).encode()
    out = subprocess.run([exe], input=stdin, stdout=subprocess.PIPE, check=True).stdout.decode().split('\n')
    result = []
    for g, (plan, index), line in zip(rows, plans, out):
        status, branch, inside = (int(x) for x in line.split())
        shape, _, variant = plan.partition(' : ')
        assert status == nat.KB_OK and index is not None, (g.name, plan)
        result.append((g, [int(x) for x in shape.split()], [int(x) for x in variant.split()], index, branch, inside))
    return result
