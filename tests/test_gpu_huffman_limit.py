"""The length limit of the Huffman codes on the MI355X: the shared cases of tests/huffman_limit_cases.py through the
real library."""
import pytest

import huffman_limit_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,level", cases.ONE_BLOCK)
def test_limited_code_one_block(hip_lib, oracle, name, level):
    cases.check_one_block(hip_lib, oracle, name, level)


@pytest.mark.parametrize("name,level", cases.PLACED)
def test_limited_code_among_ordinary_ones(hip_lib, oracle, name, level):
    cases.check_placement(hip_lib, oracle, name, level)
