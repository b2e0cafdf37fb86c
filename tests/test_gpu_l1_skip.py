"""k_mparse's step over candidate-less positions on the MI355X: the shared cases of tests/l1_skip_cases.py through the
real library."""
import pytest

import l1_skip_cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group", sorted(l1_skip_cases.GROUPS))
def test_stream_vs_oracle_with_and_without_the_step(hip_lib, oracle, group):
    l1_skip_cases.check(hip_lib, oracle, group)


def test_long_runs_are_still_handed_back(hip_lib):
    l1_skip_cases.handed_back(hip_lib)
