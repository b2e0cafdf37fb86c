"""k_emit's token loop and k_hist on the MI355X: the shared cases of tests/emit_cases.py through the real library."""
import pytest

import emit_cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group", sorted(emit_cases.GROUPS))
def test_stream_vs_oracle(hip_lib, oracle, group):
    emit_cases.check(hip_lib, oracle, group)


@pytest.mark.parametrize("cls,buffer_size,level", emit_cases.SLIDES)
def test_window_slide(hip_lib, oracle, cls, buffer_size, level):
    emit_cases.check_window_slide(hip_lib, oracle, cls, buffer_size, level)


@pytest.mark.parametrize("level", (3, 6, 9))
def test_other_token_producers(hip_lib, oracle, level):
    emit_cases.check_other_levels(hip_lib, oracle, level)


def test_framing(hip_lib, oracle):
    emit_cases.check_framing(hip_lib, oracle)
