"""DEFLATE's length and offset alphabets end to end, through the CPU emulator: the shared body of tests/alphabet_cases.py."""
import pytest

import alphabet_cases as cases
import deflate_craft as dc


@pytest.mark.parametrize("fmt", ["bgzf", "mgzip"])
@pytest.mark.parametrize("code", cases.CODES)
def test_every_length_and_offset_edge_inflates(emu_lib, code, fmt):
    cases.check_decode(emu_lib, code, dc.BGZF if fmt == "bgzf" else dc.MGZIP)


@pytest.mark.parametrize("level", cases.LEVELS)
def test_every_length_and_offset_symbol_is_written(emu_lib, oracle, level):
    cases.check_encode(emu_lib, oracle, level)
