"""k_crc32 on blocks that start off a dword boundary, through the CPU emulator: the shared body of tests/crc_cases.py."""
import pytest

import crc_cases


@pytest.mark.parametrize("shape", sorted(crc_cases.SHAPES))
def test_trailers_of_misaligned_blocks(emu_lib, shape):
    assert crc_cases.misaligned_blocks(emu_lib, shape) == {"bgzf": 116, "mgzip": 32}[shape]
