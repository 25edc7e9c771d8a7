"""The instantiation of kb_step_kernel that runs a handle (gym_kilobots_amd/csrc/kb_variant.h), checked without a GPU: the
header is plain C++ and is compiled here with the system compiler.  tests/golden/variant_selection.txt records, for every
distinct selection input of a grid of 10 032 accepted configurations, the instantiation the library ran; a configuration
that moves to a different instantiation, or an instantiation that leaves the list, fails this test."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <cstdio>
#include "kb_variant.h"
using namespace kb;
static void put(const Variant &v) {
    printf("%d %d %d %d %d %d %d %d\n", v.drive, v.light, v.obj, v.fn, v.tier, v.poly, v.sense, v.sleep);
}
int main() {
    for (int i = 0; i < kb_variants.n; ++i) put(kb_variants.v[i]);
    printf("--\n");
    int s[9];
    while (scanf("%d %d %d %d %d %d %d %d %d", &s[0], &s[1], &s[2], &s[3], &s[4], &s[5], &s[6], &s[7], &s[8]) == 9) {
        const Variant v = select_variant({s[0], s[1], s[2] != 0, s[3] != 0, s[4] != 0, s[5] != 0, s[6], s[7], s[8] != 0});
        if (variant_index(v) < 0) printf("not in the list: ");
        put(v);
    }
    return 0;
}
'''


def test_selection_matches_the_recorded_instantiations(tmp_path):
    inputs, keys = [], []
    for line in open(os.path.join(ROOT, 'tests', 'golden', 'variant_selection.txt')):
        if line.startswith('#'):
            continue
        shape, key = line.split(':')
        inputs.append(shape.strip())
        keys.append(key.strip())
    src = tmp_path / 'variant.cpp'
    src.write_text(PROGRAM)
    exe = str(tmp_path / 'variant')
    subprocess.check_call(['g++', '-std=c++17', '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'gym_kilobots_amd', 'csrc'),
                           str(src), '-o', exe])
    out = subprocess.run([exe], input='\n'.join(inputs).encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split('\n')
    sep = out.index('--')
    listed, selected = out[:sep], out[sep + 1:sep + 1 + len(inputs)]
    assert len(listed) == 176 and len(set(listed)) == 176
    assert set(listed) == set(keys)         # every instantiation is reached, none beyond the list
    for shape, want, got in zip(inputs, keys, selected):
        assert got == want, 'selection input %s: %s, recorded %s' % (shape, got, want)
