"""The length limit of the Huffman codes in the CPU emulator: the shared cases of tests/huffman_limit_cases.py.  No GPU."""
import pytest

import huffman_limit_cases as cases


@pytest.mark.parametrize("name,level", cases.ONE_BLOCK)
def test_limited_code_one_block(emu_lib, oracle, name, level):
    cases.check_one_block(emu_lib, oracle, name, level)


@pytest.mark.parametrize("name,level", cases.PLACED)
def test_limited_code_among_ordinary_ones(emu_lib, oracle, name, level):
    cases.check_placement(emu_lib, oracle, name, level)
