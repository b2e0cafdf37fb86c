"""k_mparse at the turn of a pass and of a block in the CPU emulator: the shared cases of tests/turnover_cases.py.
No GPU.  (The emulator runs the ticket loop too: a block that nobody claims shows here as a stream that differs.)"""
import pytest

import turnover_cases


@pytest.mark.parametrize("group", sorted(turnover_cases.GROUPS))
def test_stream_vs_oracle(emu_lib, oracle, group):
    turnover_cases.check(emu_lib, oracle, group)
