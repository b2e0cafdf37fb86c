"""libdeflate's parsing rules (gzp_amd/csrc/gzpx_policy.h) on the MI355X: the shared bodies of tests/policy_cases.py
through the real library."""
import pytest

import policy_cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("level", policy_cases.ALPHABET_LEVELS)
def test_min_len_by_alphabet(hip_lib, oracle, level):
    policy_cases.min_len_by_alphabet(hip_lib, oracle, level)


@pytest.mark.parametrize("level", policy_cases.SHORT_LEVELS)
def test_short_scan(hip_lib, oracle, level):
    policy_cases.short_scan(hip_lib, oracle, level)


@pytest.mark.parametrize("level", policy_cases.RECALC_LEVELS)
def test_recalculation(hip_lib, oracle, level):
    policy_cases.recalculation(hip_lib, oracle, level)
