"""The fields of lines through the CPU emulator (a device pointer is a host pointer there): the shared bodies of
tests/field_cases.py, every byte and offset compared with what split and join give on zlib's inflate of the same
members."""
import field_cases


def test_rule(emu_lib):
    field_cases.rule(emu_lib)


def test_edges_of_the_walk(emu_lib):
    field_cases.edges(emu_lib)


def test_ranges(emu_lib):
    field_cases.ranges(emu_lib)


def test_close_the_loop(emu_lib):
    field_cases.close_the_loop(emu_lib)


def test_capacity(emu_lib):
    field_cases.capacity(emu_lib)


def test_errors(emu_lib):
    field_cases.errors(emu_lib)


def test_damaged_member(emu_lib):
    field_cases.damaged(emu_lib)
