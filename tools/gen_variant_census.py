"""Writes tests/golden/variant_census.txt: for every entry of kb_variants (gym_kilobots_amd/csrc/kb_variant.h) the smallest
configuration that selects it and still has contacts, found by a census of plan_launch on the host.

    python tools/gen_variant_census.py

Run it again when the list or the selection rule changes; tests/test_variant_census_cpu.py says which rows no longer hold."""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import variant_census as VC      # noqa: E402

NCELL = 2494                                 # the 2 x 1.5 m arena
GENERAL = [2, 3, 4]                          # GRADIENT, MOMENTUM, COMPOSITE in turn (index mod 3)

HEADER = '''# One configuration per instantiation of kb_step_kernel (gym_kilobots_amd/csrc/kb_variant.h: kb_variants), in list order:
# the smallest shape that selects it and still has contacts (tools/gen_variant_census.py wrote this file).
#   no objects, tier 2: 40 kilobots at kb_create's own width; tier 0: 128 kilobots with kb_set_block_threads(64)
#   objects (2 discs / 2 boxes), tier 1: 40 kilobots; tier 0: 129 kilobots
#   mixed drive laws (2 boxes), tier 1 / tier 3: 40 / 129 kilobots;  fixed-size kernels: 1024 kilobots
#   2 x 1.5 m arena (2494 cells), contact_capacity 0; light class GENERAL: GRADIENT, MOMENTUM, COMPOSITE by index mod 3
# num_bots num_objects num_fixtures all_discs drive_mode light_type sense allow_sleep ncell contact_capacity threads (0: kb_create)
#   : index in kb_variants : DRIVE LIGHT OBJ FN TIER POLY SENSE SLEEP
'''


def inputs_of(i, v):
    drive, light, obj, fn, tier, poly, sense, sleep = v
    lt = GENERAL[i % 3] if light == 99 else light
    if fn == 1024:
        N, M, threads = 1024, 2 if obj else 0, 0
    elif drive == 5:
        N, M, threads = {1: 40, 3: 129}[tier], 2, 0
    elif obj:
        N, M, threads = {1: 40, 0: 129}[tier], 2, 0
    else:
        N, M, threads = {2: (40, 0, 0), 0: (128, 0, 64)}[tier]
    discs = int(M > 0 and not poly)
    return [N, M, M, discs, drive, lt, int(sense), int(sleep), NCELL, 0, threads]


def main():
    with tempfile.TemporaryDirectory() as d:
        listed, _ = VC.host_census(d, [])
        rows = [inputs_of(i, v) for i, v in enumerate(listed)]
        _, selected = VC.host_census(d, rows)
    lines = []
    for i, (r, v, (status, got)) in enumerate(zip(rows, listed, selected)):
        if status != 0 or got != i:
            sys.exit('instantiation %d %s: inputs %s select %d (status %d); adapt inputs_of()' % (i, v, r, got, status))
        lines.append('%s : %d : %s\n' % (' '.join(map(str, r)), i, ' '.join(map(str, v))))
    with open(VC.CENSUS, 'w') as f:
        f.write(HEADER)
        f.writelines(lines)
    print('%s: %d rows' % (VC.CENSUS, len(lines)))


if __name__ == '__main__':
    main()
