"""The short forms of the position sweep (gym_kilobots_amd/csrc/kb_exact.h) give the bits of the IEEE operation for EVERY
seed their instruction may return, not for one chip's table: tests/exact_forms_check.cpp, compiled here with the system
compiler, enumerates them.

    division     a / K by Markstein's step: all 2^23 mantissas x every exponent |C| can take (2^-34 .. 0.2) x both signs, and
                 both zeros, for the default configuration's two K, a K whose mantissa is all ones and a power of two
    reciprocal   1 / x: all 2^23 mantissas but the one the guard keeps away x every float within 1 ulp of 1 / x (v_rcp_f32)
    square root  sqrt(x): every x of a binade inside the guard x every pair of floats within 1 ulp of sqrt(x) (v_sqrt_f32)
                 and of 1 / sqrt(x) (v_rsq_f32: the ISA documents 1 ulp for all three)

The forms are invariant under scaling by a power of two (four for the root) while nothing leaves the normal range, so one
binade would do; the binades at both ends of the guard and the ones the headline's contacts live in are run as well.
What the guard leaves out -- the four largest mantissas of every binade of dd -- is shown to be necessary (the two forms DO
miss there) and sufficient (no dd inside the guard has a root with an all-ones mantissa)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'gym_kilobots_amd', 'csrc')

DD_MIN_EXP, DD_MAX_EXP = -40, 39            # kb_exact.h: 2^-40 <= dd < 2^40
MANT_MAX = 0x7FFFFC                         # ... and mantissa below this
C_EXPS = 32                                 # exponents -34 .. -3 of |C|


@pytest.fixture(scope='module')
def checker(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('exact') / 'exact_forms_check')
    subprocess.check_call([cxx, '-O2', '-std=c++17', '-ffp-contract=off', '-pthread', '-I', CSRC,
                           os.path.join(ROOT, 'tests', 'exact_forms_check.cpp'), '-o', exe])

    def run(form, *cases):
        r = subprocess.run([exe, form] + [str(c) for c in cases], stdout=subprocess.PIPE, universal_newlines=True)
        rows = re.findall(r'^(\S+) (\S+) checked (\d+) mismatches (\d+)$', r.stdout, re.M)
        assert len(rows) == len(cases) and r.returncode in (0, 1), r.stdout
        print(r.stdout)
        return [(int(n), int(bad)) for _, _, n, bad in rows], r.returncode
    return run


def header_constants():
    src = open(os.path.join(CSRC, 'kb_exact.h')).read()
    get = lambda name: int(re.search(name + r'\s*=\s*(-?\w+?)u?\s*[;,]', src).group(1), 0)     # noqa: E731
    return {k: get(k) for k in ('KB_EXACT_DD_MIN_BITS', 'KB_EXACT_DD_MAX_BITS', 'KB_EXACT_MANT_MAX', 'KB_EXACT_C_EXP_MIN', 'KB_EXACT_C_EXP_MAX')}


def default_divisors():
    """im_bot + im_bot and 0 + im_bot of the default configuration, by the fp32 expressions of kb_create"""
    c = O.default_config(1, 16)
    f = np.float32
    r = f(c.bot_radius) * f(25.0)
    m = f(c.bot_density) * f(3.14159265359) * r * r
    im = f(1.0) / m
    return [int((im + im).view(np.uint32)), int((f(0.0) + im).view(np.uint32))]


def test_the_guard_is_the_range_the_checks_below_cover():
    k = header_constants()
    bits = lambda e: (e + 127) << 23     # noqa: E731
    assert k['KB_EXACT_DD_MIN_BITS'] == bits(DD_MIN_EXP) and k['KB_EXACT_DD_MAX_BITS'] == bits(DD_MAX_EXP + 1)
    assert k['KB_EXACT_MANT_MAX'] == MANT_MAX
    assert (k['KB_EXACT_C_EXP_MIN'], k['KB_EXACT_C_EXP_MAX']) == (-34, -3) and 2.0 ** -3 <= 0.2 < 2.0 ** -2
    # the headline's contacts: lengths 0.4 .. 0.9 world units between kilobot centres, dd = len^2 accordingly
    for length in (0.4, 0.9):
        dd = np.float32(length * length)
        assert 2.0 ** DD_MIN_EXP <= dd < 2.0 ** (DD_MAX_EXP + 1)
        assert -3 <= int(np.floor(np.log2(dd))) <= -1
    # ... and B2_EPSILON, the threshold of the branch for coincident centres, lies below every len = sqrt(dd) of the guard
    assert 1.19209290e-07 < 2.0 ** (DD_MIN_EXP / 2)


def test_division_by_the_two_constants(checker):
    ks = default_divisors() + [0x3FFFFFFF, 0x40000000]       # + all-ones mantissa (Markstein's hard case), + a power of two
    assert len(set(ks)) == 4
    rows, rc = checker('div', *map(hex, ks))
    assert rc == 0 and all(n == 2 * C_EXPS * 2 ** 23 + 2 and bad == 0 for n, bad in rows), rows


def test_reciprocal_from_any_seed_within_one_ulp(checker):
    # len = sqrt(dd): the two ends of the guard, the headline's binades (0.4 .. 0.9), and [1, 2)
    rows, rc = checker('rcp', -20, 19, -2, -1, 0)
    assert rc == 0 and all(n >= 2 * (2 ** 23 - 1) and bad == 0 for n, bad in rows), rows


def test_square_root_from_any_pair_of_seeds_within_one_ulp(checker):
    exps = [DD_MIN_EXP, DD_MIN_EXP + 1, -3, -2, -1, 0, 1, DD_MAX_EXP - 1, DD_MAX_EXP]
    rows, rc = checker('sqrt', *exps)
    assert rc == 0 and all(n >= 4 * (MANT_MAX - 1) and bad == 0 for n, bad in rows), rows


def test_the_guard_keeps_the_all_ones_length_away(checker):
    exps = [DD_MIN_EXP, DD_MIN_EXP + 1, -3, -2, -1, 0, 1, DD_MAX_EXP - 1, DD_MAX_EXP]
    rows, rc = checker('guard', *exps)
    assert rc == 0 and all(n == MANT_MAX and bad == 0 for n, bad in rows), rows
    rows, rc = checker('guard', DD_MIN_EXP - 1, DD_MAX_EXP + 1)       # outside: nothing is inside the guard
    assert rc == 0 and all(n == 0 for n, _ in rows), rows


def test_the_excluded_mantissas_are_excluded_for_a_reason(checker):
    """Without the mantissa clause both forms miss (a compliant seed exists that lands on a tie): the guard is not decoration."""
    rows, rc = checker('unguarded', 0, 1)
    assert rc == 1 and sum(bad for _, bad in rows) > 0, rows


def test_the_forms_that_were_left_out_do_miss(checker):
    """DESIGN.md section 3 quotes these counts: v_rsq_f32(dd) as the seed of 1 / len (up to 2 ulp from 1 / RN(sqrt(dd))) and the
    root from dd * rsq alone are not exact for every compliant seed, so the kernel issues v_rcp_f32 and v_sqrt_f32."""
    rows, rc = checker('rcp_rsq', 0, 1)
    assert rc == 1 and [bad for _, bad in rows] == [7, 3], rows
    rows, rc = checker('sqrt_rsq', 0, 1)
    assert rc == 1 and [bad for _, bad in rows] == [0, 1], rows


def test_kb_create_checks_the_division_for_its_handle():
    """The default configuration's two K pass the check of kb_create (no GPU needed): the handle multiplies."""
    import ctypes as C
    from gym_kilobots_amd import _native as nat
    lib = nat.load()
    cfg = nat.default_config(1, 16, O.DRIVE_VELOCITY, O.LIGHT_NONE)
    h = C.c_void_p()
    assert lib.kb_create(C.byref(cfg), C.byref(h)) == nat.KB_OK
    assert lib.kb_exact_division(h) == 1
    lib.kb_destroy(h)
