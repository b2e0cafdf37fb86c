"""DEFLATE's length and offset alphabets end to end, on the MI355X: the shared body of tests/alphabet_cases.py."""
import pytest

import alphabet_cases as cases
import deflate_craft as dc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fmt", ["bgzf", "mgzip"])
@pytest.mark.parametrize("code", cases.CODES)
def test_every_length_and_offset_edge_inflates(hip_lib, code, fmt):
    cases.check_decode(hip_lib, code, dc.BGZF if fmt == "bgzf" else dc.MGZIP)


@pytest.mark.parametrize("level", cases.LEVELS)
def test_every_length_and_offset_symbol_is_written(hip_lib, oracle, level):
    cases.check_encode(hip_lib, oracle, level)
