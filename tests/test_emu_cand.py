"""k_candidates' interior and clamped bodies in the CPU emulator: the shared cases of tests/cand_cases.py.  No GPU.
(The emulator runs the ticket loop too: a turn that nobody hands on shows here as a test that never ends.)"""
import pytest

import cand_cases


@pytest.mark.parametrize("group", sorted(cand_cases.GROUPS))
def test_stream_vs_oracle_in_three_ways(emu_lib, oracle, group):
    cand_cases.check(emu_lib, oracle, group)
