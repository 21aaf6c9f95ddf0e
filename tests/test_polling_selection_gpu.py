"""
The HIP polling kernel on the constructed cases of tests/polling_cases.py: every branch of its one-pass plane selection (the per-lane
state machine, the merge over four wavefronts, the four-way final resolution) and its three forms (1, 2 or 4 planes per loop iteration,
reached by N alone) against oracle/polling.c, which selects the naive way.  Bar: the plane index exact, keypoints, keyplanes and
residuals bit for bit (helpers.bits_equal: the GPU and x86 give NaN different sign bits).  No tolerance is involved.

tests/test_polling_selection_cpu.py shows, on the reference alone, that each case reaches the branch it is named for.
"""
import numpy as np
import pytest

import helpers
import polling_cases as pc
from keras_retinanet_3D.utils import gpp_utils

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', pc.NAMES)
def test_hip_polling_selection_case_against_oracle(name, oracle_lib):
    case = pc.get(name)
    ref = helpers.c_oracle_poll(oracle_lib, *case.args(), thr=case.thr)
    got = gpp_utils.fit_road_planes(*[a.copy() for a in case.args()], return_index=True, threshold=case.thr)     # (the cached case is read-only)
    for c in case.claims:                                  # the rows the case was built for, by name: a clearer message than the array's
        if 'index' in c:
            assert int(got[3][c['row']]) == c['index'], '{} row {}: {}'.format(name, c['row'], c)
    assert np.array_equal(got[3], ref[3])
    for a, b in zip(got[:3], ref[:3]):
        assert helpers.bits_equal(a, b)
