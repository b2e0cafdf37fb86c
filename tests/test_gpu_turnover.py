"""k_mparse at the turn of a pass and of a block on the MI355X: the shared cases of tests/turnover_cases.py through
the real library."""
import pytest

import turnover_cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group", sorted(turnover_cases.GROUPS))
def test_stream_vs_oracle(hip_lib, oracle, group):
    turnover_cases.check(hip_lib, oracle, group)
