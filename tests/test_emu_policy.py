"""libdeflate's parsing rules (gzp_amd/csrc/gzpx_policy.h) through the CPU emulator: the shared bodies of
tests/policy_cases.py."""
import pytest

import policy_cases


@pytest.mark.parametrize("level", policy_cases.ALPHABET_LEVELS)
def test_min_len_by_alphabet(emu_lib, oracle, level):
    policy_cases.min_len_by_alphabet(emu_lib, oracle, level)


@pytest.mark.parametrize("level", policy_cases.SHORT_LEVELS)
def test_short_scan(emu_lib, oracle, level):
    policy_cases.short_scan(emu_lib, oracle, level)


@pytest.mark.parametrize("level", policy_cases.RECALC_LEVELS)
def test_recalculation(emu_lib, oracle, level):
    policy_cases.recalculation(emu_lib, oracle, level)
