"""gzpx_checksum_batch_device on the MI355X: the shared bodies of tests/checksum_cases.py through the real library."""
import pytest

import checksum_cases
from checksum_cases import KINDS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("what", ["random", "ff", "zero"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_values(hip_lib, kind, what):
    checksum_cases.known_answers()
    checksum_cases.values(hip_lib, KINDS[kind], what)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_seeds(hip_lib, kind):
    checksum_cases.seeds(hip_lib, KINDS[kind])


def test_both_table_shapes_and_the_zip_case(hip_lib):
    checksum_cases.zip_case(hip_lib)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_overlap_and_order(hip_lib, kind):
    checksum_cases.overlap_and_order(hip_lib, KINDS[kind])


def test_invalid_entries_and_arguments(hip_lib):
    checksum_cases.invalid(hip_lib)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_ragged(hip_lib, kind):
    # (the CRC-32C reference is Python: its long entry stays at a few tiles)
    checksum_cases.ragged(hip_lib, KINDS[kind], big=0 if kind == "crc32c" else (64 << 20) + 5, widths=(0, 1000))


def test_entries_beyond_4_gib(hip_lib):
    checksum_cases.beyond_4gib(hip_lib)


def test_stream_order(hip_lib):
    checksum_cases.stream_order(hip_lib)
