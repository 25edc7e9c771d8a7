"""The short forms of the position sweep with the seeds of THIS chip (v_sqrt_f32, v_rsq_f32, v_rcp_f32): kb_exact_selftest
runs each form over all 2^32 bit patterns on the device and counts, per form, the operands inside its guard and the
results that differ in a bit from the compiler's sqrtf(x), 1.0f / x and a / K (tests/test_exact_forms_cpu.py proves the
same for every seed the ISA allows)."""
import ctypes as C

import pytest
import torch

from gym_kilobots_amd import _native as nat
from gym_kilobots_amd.sim import KilobotSim

pytestmark = pytest.mark.gpu

MANT_MAX = 0x7FFFFC      # kb_exact.h: mantissas of dd inside the guard, 80 binades of them
C_EXPS = 32              # exponents of |C|


def test_every_wired_form_matches_the_compiler_on_every_bit_pattern():
    sim = KilobotSim(1, 16)
    assert sim._lib.kb_exact_division(sim._h) == 1
    counts = torch.full((6,), -1, dtype=torch.int64, device=sim.device)
    nat.check(sim._lib.kb_exact_selftest(sim._h, C.c_void_p(counts.data_ptr()), sim._stream()), 'kb_exact_selftest')
    torch.cuda.synchronize()
    n_sqrt, bad_sqrt, n_rcp, bad_rcp, n_div, bad_div = counts.tolist()
    print('checked / mismatches: sqrt %d / %d, rcp %d / %d, div %d / %d' % (n_sqrt, bad_sqrt, n_rcp, bad_rcp, n_div, bad_div))
    assert n_sqrt == 80 * MANT_MAX                      # 2^-40 <= dd < 2^40
    assert n_rcp == 40 * (2 ** 23 - 1)                  # 2^-20 <= len < 2^20, mantissa not all ones
    assert n_div == 2 * (2 * C_EXPS * 2 ** 23 + 2)      # both K: both signs of 2^-34 <= |a| < 2^-2, and both zeros
    assert (bad_sqrt, bad_rcp, bad_div) == (0, 0, 0)
    sim.close()
