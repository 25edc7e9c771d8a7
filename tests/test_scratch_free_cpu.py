"""Generated-code check (no GPU needed): the step kernels without objects use no scratch memory.

A private variable that is addressed through a selected or indexed pointer stays in scratch memory although the kernel
spills no vector register (the partner list of the contact search did): every access is then a trip
to L2 that the wave waits for.  The kernel metadata of the assembly that build() keeps next to the objects it links
(where build.lint_codegen() reads) says so: `.private_segment_fixed_size` is the scratch size per lane,
`.vgpr_spill_count` the registers the allocator spilled.  Kernels with objects keep genuine private arrays and are not
held to this."""
import glob
import os
import re

import pytest

from gym_kilobots_amd import build as kb_build

HEADLINE = '_ZN2kb14kb_step_kernelILi0ELi0ELb0ELi1024ELi0ELb1ELb0ELb0EEEvNS_6ParamsE'     # kb_step_kernel<0, 0, false, 1024, 0, true, false, false>
FIELDS = ('private_segment_fixed_size', 'vgpr_spill_count', 'vgpr_count')
STEP_KERNEL = re.compile(r'^_ZN2kb14kb_step_kernelIL[ij]\d+EL[ij]\d+ELb([01])E')       # third template argument: objects


@pytest.fixture(scope='module')
def kernels():
    """{kernel name: {field: int}} of every kernel unit of the shipped library"""
    kb_build.build()
    out = {}
    units = [s for s in kb_build.sources() if os.path.basename(s).startswith('kb_inst_')]
    assert len(units) == 12
    newest = max(os.path.getmtime(d) for d in glob.glob(os.path.join(kb_build.CSRC, '*')))
    for src in units:
        path = kb_build._device_asm(os.path.join(kb_build.HERE, '_obj', 'rel'), src)
        assert os.path.getmtime(path) >= newest, '%s is older than the sources' % path
        text = open(path).read()
        name = None
        for line in text[text.rindex('amdhsa.kernels:'):].split('\n'):        # the metadata note at the end of the unit
            m = re.match(r'\s+(?:- )?\.(\w+):\s+(\S+)\s*$', line)
            if not m:
                continue
            if m.group(1) == 'name' and m.group(2).startswith('_Z'):
                name = m.group(2)
                out[name] = {}
            elif name is not None and m.group(1) in FIELDS:
                out[name][m.group(1)] = int(m.group(2))
    return out


def test_every_step_kernel_reports_its_resources(kernels):
    step = {n: r for n, r in kernels.items() if STEP_KERNEL.match(n)}
    assert len(step) == 176, len(step)
    assert all(set(r) == set(FIELDS) for r in step.values())


def test_step_kernels_without_objects_use_no_scratch(kernels):
    held, bad = 0, []
    for n, r in sorted(kernels.items()):
        m = STEP_KERNEL.match(n)
        if not m or m.group(1) == '1' or r['vgpr_spill_count'] != 0:
            continue
        held += 1
        if r['private_segment_fixed_size'] != 0:
            bad.append('%s: %d B of scratch per lane with no spilled VGPR' % (n, r['private_segment_fixed_size']))
    print('%d step kernels without objects and without VGPR spills' % held)
    assert held > 0
    assert not bad, '\n'.join(bad)


def test_the_headline_kernel_uses_no_scratch(kernels):
    r = kernels[HEADLINE]
    assert r['vgpr_spill_count'] == 0 and r['private_segment_fixed_size'] == 0, r
    assert r['vgpr_count'] <= 80, r       # three envs per CU need <= 80 VGPRs
