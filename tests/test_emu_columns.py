"""The numeric columns of lines through the CPU emulator (a device pointer is a host pointer there): the shared bodies of
tests/column_cases.py, every cell and status byte compared with a Python model of the rules on zlib's inflate of the same
members."""
import column_cases


def test_grammar(emu_lib):
    column_cases.grammar(emu_lib)


def test_edges_of_the_walk(emu_lib):
    column_cases.edges(emu_lib)


def test_ranges(emu_lib):
    column_cases.ranges(emu_lib)


def test_capacity(emu_lib):
    column_cases.capacity(emu_lib)


def test_errors(emu_lib):
    column_cases.errors(emu_lib)


def test_damaged_member(emu_lib):
    column_cases.damaged(emu_lib)


def test_close_the_loop(emu_lib):
    column_cases.close_the_loop(emu_lib)
