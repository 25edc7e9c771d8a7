"""The census table (tests/golden/variant_census.txt) without a GPU: its rows map one to one onto the library's list of
step-kernel instantiations (kb_launch.h compiled with the system compiler), and the scene that tests/variant_census.py
makes of every row is not vacuous on the oracle -- it has contacts, neighbours in sensing range, kilobots on the
objects, and kilobots (objects) that fall asleep wherever the drive law lets them rest.
tests/test_variant_census_gpu.py runs the same scenes on the device."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import variant_census as VC

ROWS = VC.rows()


def test_rows_select_every_instantiation_exactly_once(tmp_path):
    assert len(ROWS) == VC.NUM_VARIANTS
    listed, selected = VC.host_census(tmp_path, [r[0] for r in ROWS])
    assert len(listed) == VC.NUM_VARIANTS and len(set(listed)) == VC.NUM_VARIANTS
    redo = []
    for i, ((inputs, index, variant), (status, got)) in enumerate(zip(ROWS, selected)):
        if not (index == i and status == 0 and got == i and variant == listed[i]):
            redo.append('row %d (%s): records index %d %s, selects %d (status %d); the list has %s there'
                        % (i, ' '.join(map(str, inputs)), index, variant, got, status, listed[i]))
    assert not redo, 'kb_variants or the selection changed; redo these rows (tools/gen_variant_census.py):\n' + '\n'.join(redo)
    assert sorted(got for _, got in selected) == list(range(VC.NUM_VARIANTS))
    # the smallest shapes: nothing but the eight fixed-size kernels needs more than 129 kilobots
    big = [i for i, (inputs, _, variant) in enumerate(ROWS) if inputs[0] > 129]
    assert big == [i for i, v in enumerate(listed) if v[3] == 1024] and len(big) == 8
    # 2 x 1.5 m arena, derived contact capacity; every model of the GENERAL light class is used
    assert all(inputs[8] == 2494 and inputs[9] == 0 for inputs, _, _ in ROWS)
    assert {inputs[5] for inputs, _, v in ROWS if v[1] == 99} == {O.LIGHT_GRADIENT, O.LIGHT_MOMENTUM, O.LIGHT_COMPOSITE}
    assert len({VC.row_id(r) for r in ROWS}) == VC.NUM_VARIANTS


@pytest.mark.parametrize('row', ROWS, ids=VC.row_id)
def test_scene_is_not_vacuous_on_the_oracle(row):
    s = VC.scene(row)
    osim = VC.oracle_sim(s)
    contacts = neighbours = on_object = slept = objects_slept = False
    for k, step in enumerate(s.steps):
        VC.oracle_step(osim, step)
        assert int(osim.status.max()) == 0, 'substep %d: status %s' % (k, osim.status)
        contacts = contacts or int(osim.ws_cnt.astype(np.int64).sum(1).min()) > 0
        neighbours = neighbours or int(osim.nbr_count.max()) > 0
        if s.objects is not None and not on_object:
            on_object = any(osim.count_contacts(e, True)[2] > 0 for e in range(s.E))
        if s.sleeps is not None:
            slept = slept or bool((osim.sleep_time < 0).any())
            objects_slept = objects_slept or (s.objects is not None and bool((osim.osleep < 0).any()))
    assert contacts, 'no substep with contacts in every env'
    if 'nbr_count' in s.fields:
        assert neighbours, 'nobody in sensing range'
    if s.objects is not None:
        assert on_object, 'no kilobot touches an object'
    if s.sleeps is not None:
        # (False: the drive law keeps every kilobot moving; a change of that is to be noticed as well)
        assert slept == s.sleeps, 'kilobots %s asleep' % ('never fell' if s.sleeps else 'fell')
    if s.objects_sleep:
        assert objects_slept, 'no object fell asleep'
