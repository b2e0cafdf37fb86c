"""Reads by line through the CPU emulator (a device pointer is a host pointer there): the shared bodies of
tests/line_cases.py, every table, offset and byte compared with what numpy finds in zlib's inflate of the same members."""
import line_cases


def test_table(emu_lib, oracle):
    line_cases.table(emu_lib, oracle)


def test_offsets(emu_lib, oracle):
    line_cases.offsets(emu_lib, oracle)


def test_reads(emu_lib, oracle):
    line_cases.reads(emu_lib, oracle)


def test_errors(emu_lib, oracle):
    line_cases.errors(emu_lib, oracle)


def test_only_needed_members_are_touched(emu_lib):
    line_cases.touched(emu_lib)
