"""k_crc32 on blocks that start off a dword boundary, on the MI355X: the shared body of tests/crc_cases.py."""
import pytest

import crc_cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", sorted(crc_cases.SHAPES))
def test_trailers_of_misaligned_blocks(hip_lib, shape):
    assert crc_cases.misaligned_blocks(hip_lib, shape) == {"bgzf": 116, "mgzip": 32}[shape]
