"""gzpx_checksum_batch_device through the CPU emulator (a device pointer is a host pointer there): the shared bodies of
tests/checksum_cases.py, the cross product of lengths and misalignments thinned to three misalignments."""
import pytest

import checksum_cases
from checksum_cases import KINDS


def test_references_on_known_answers():
    checksum_cases.known_answers()


@pytest.mark.parametrize("what", ["random", "ff", "zero"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_values(emu_lib, kind, what):
    checksum_cases.values(emu_lib, KINDS[kind], what, misalignments=(0, 3, 13))


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_seeds(emu_lib, kind):
    checksum_cases.seeds(emu_lib, KINDS[kind])


def test_both_table_shapes_and_the_zip_case(emu_lib):
    checksum_cases.zip_case(emu_lib, small=True)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_overlap_and_order(emu_lib, kind):
    checksum_cases.overlap_and_order(emu_lib, KINDS[kind])


def test_invalid_entries_and_arguments(emu_lib):
    checksum_cases.invalid(emu_lib)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_ragged(emu_lib, kind):
    # two launch widths: hundreds of entries to a workgroup, and fewer tiles to a workgroup than a long entry has
    checksum_cases.ragged(emu_lib, KINDS[kind], widths=(7, 3001))


def test_no_read_outside_the_input(emu_lib):
    checksum_cases.no_read_outside_input(emu_lib)
