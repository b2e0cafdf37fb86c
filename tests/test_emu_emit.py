"""k_emit's token loop and k_hist in the CPU emulator: the shared cases of tests/emit_cases.py.  No GPU."""
import pytest

import emit_cases


@pytest.mark.parametrize("group", sorted(emit_cases.GROUPS))
def test_stream_vs_oracle(emu_lib, oracle, group):
    emit_cases.check(emu_lib, oracle, group)


@pytest.mark.parametrize("cls,buffer_size,level", emit_cases.SLIDES)
def test_window_slide(emu_lib, oracle, cls, buffer_size, level):
    emit_cases.check_window_slide(emu_lib, oracle, cls, buffer_size, level)


@pytest.mark.parametrize("level", (3, 6, 9))
def test_other_token_producers(emu_lib, oracle, level):
    emit_cases.check_other_levels(emu_lib, oracle, level)


def test_framing(emu_lib, oracle):
    emit_cases.check_framing(emu_lib, oracle)
