"""k_mparse's step over candidate-less positions in the CPU emulator: the shared cases of tests/l1_skip_cases.py.  No GPU."""
import pytest

import l1_skip_cases


@pytest.mark.parametrize("group", sorted(l1_skip_cases.GROUPS))
def test_stream_vs_oracle_with_and_without_the_step(emu_lib, oracle, group):
    l1_skip_cases.check(emu_lib, oracle, group)


def test_long_runs_are_still_handed_back(emu_lib):
    l1_skip_cases.handed_back(emu_lib)
