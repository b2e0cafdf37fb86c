"""k_candidates' interior and clamped bodies on the MI355X: the shared cases of tests/cand_cases.py through the real
library."""
import pytest

import cand_cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group", sorted(cand_cases.GROUPS))
def test_stream_vs_oracle_in_three_ways(hip_lib, oracle, group):
    cand_cases.check(hip_lib, oracle, group)
