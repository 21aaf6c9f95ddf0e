"""
The census of tests/polling_cases.py (no GPU): every constructed case shows, on the reference alone (oracle/polling_np.py), the branch of
csrc/poll.hip's one-pass selection it was built for -- the class of the final resolution, the planted index, the level rises along a
lane, the lane / wavefront / iteration of the answer.  If a builder stops producing its branch, this file fails, not the GPU test
silently.  The same cases pin oracle/polling.c to oracle/polling_np.py (index exact, values bit for bit), NaN, sentinel and threshold
inputs included, since the C form is what the GPU test compares the kernel with.
"""
import os
import re

import numpy as np
import pytest

import helpers
import polling_cases as pc

FINALS = ('lt100', 'eq100_sentinel_first', 'eq100_imin_first', 'eq100_no_sentinel', 'gt100_sentinel', 'nonfinite_sentinel',
          'gt100_no_sentinel', 'nothing')


@pytest.mark.parametrize('name', pc.NAMES)
def test_case_reaches_its_branch_and_the_two_oracles_agree(name, oracle_lib):
    case = pc.get(name)
    cen = pc.census(case)
    assert pc.failed_claims(case, cen) == []
    ref = case.numpy_oracle()
    # the census's literal rule is the oracle's, and the one-pass resolution (rmin, imin, i100 -> index) derives the same answer
    assert np.array_equal(cen['index'], ref[3])
    assert np.array_equal(cen['model_index'], ref[3])
    got = helpers.c_oracle_poll(oracle_lib, *case.args(), thr=case.thr)
    assert np.array_equal(got[3], ref[3])
    for a, b in zip(got[:3], ref[:3]):
        assert helpers.bits_equal(a, b)


def test_every_branch_has_an_asserted_case():
    """ one claimed row at least per class of the final resolution (`== 100` in both orders and without a sentinel, `-> 0` included), the
    sentinel behind a level rise, a staircase of >= 3 rises, an answer in every wavefront and in a later iteration of every form """
    claimed = {}
    for name in pc.NAMES:
        for c in pc.get(name).claims:
            if 'final' in c:
                claimed.setdefault(c['final'], []).append(name)
    assert set(claimed) == set(FINALS), sorted(set(FINALS) - set(claimed))
    for n in pc.FORM_N:
        assert any(c.get('min_rises', 0) >= 3 for c in pc.get('staircase_{}'.format(n)).claims)
        assert any('stale_minimum_on_lane' in c for c in pc.get('stale_minimum_{}'.format(n)).claims)      # what a rise must forget
        risen = [c for c in pc.get('sentinel_wins_{}'.format(n)).claims if 'rises_on_lane' in c]
        assert {c['index'] for c in risen} == {0, 3 * pc.WAVE + 8}          # i100 = tid after a rise, in wavefronts 0 and 3
        where = [pc.position(c['index'], n) for name in ('planted', 'duplicated', 'sentinel_wins')
                 for c in pc.get('{}_{}'.format(name, n)).claims]
        assert {w for _, w, _, _ in where} == {0, 1, 2, 3}
        assert max(it for _, _, it, _ in where) >= 1
        assert {slot for _, _, _, slot in where} == set(range(pc.unroll_for(n)))


def test_sizes_reach_every_form_and_every_tail():
    """ the table of sizes against the rule that picks the form, and that rule against the text of csrc/poll.hip """
    assert sorted(pc.SIZES) == [1, 2, 4] and sorted({pc.unroll_for(n) for n in pc.FORM_N}) == [1, 2, 4]
    for form, sizes in pc.SIZES.items():
        assert all(pc.unroll_for(n) == form for n in sizes)
        assert all('size_{}'.format(n) in pc.BUILDERS for n in sizes)
        # slots of the last loop iteration that lie wholly past the end, and a last round that fills only some lanes
        empty_slots = {(form - (-(-n // pc.LANES)) % form) % form for n in sizes}
        assert empty_slots >= set(range(form))
        assert any(n % pc.LANES == 1 for n in sizes) and any(n % pc.LANES == pc.LANES - 1 for n in sizes)
    assert max(pc.SIZES[1]) == 4 * pc.LANES - 1 and min(pc.SIZES[2]) == 4 * pc.LANES         # both sides of each threshold
    assert max(pc.SIZES[2]) == 16 * pc.LANES - 1 and min(pc.SIZES[4]) == 16 * pc.LANES
    src = open(os.path.join(helpers.ROOT, 'ground-plane-polling_amd', 'csrc', 'poll.hip')).read()
    assert re.search(r'constexpr int kThreads = 64 \* kWaves;', src) and re.search(r'constexpr int kWaves = 4;', src)
    assert re.search(r'N >= 16 \* kThreads \? 4 : \(N >= 4 \* kThreads \? 2 : 1\)', src), 'the rule that picks the form moved: update polling_cases.unroll_for and SIZES'


def test_cases_stay_inside_the_gpu_budget():
    """ D <= 8, B <= 14, N <= 6143 per call """
    for name in pc.NAMES:
        case = pc.get(name)
        B, D = case.boxes.shape[:2]
        assert B <= 14 and D <= 8 and case.N <= 6143, name
