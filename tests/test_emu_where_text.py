"""The selection of lines by the text of their fields through the CPU emulator (a device pointer is a host pointer there):
the shared bodies of tests/where_text_cases.py, every run and count compared with a Python model of the rules on zlib's
inflate of the same members."""
import where_text_cases


def test_operators(emu_lib):
    where_text_cases.operators(emu_lib)


def test_edges_of_the_walk(emu_lib):
    where_text_cases.edges(emu_lib)


def test_mixed(emu_lib):
    where_text_cases.mixed(emu_lib)


def test_most_terms(emu_lib):
    where_text_cases.most(emu_lib)


def test_equivalence(emu_lib):
    where_text_cases.equivalence(emu_lib)


def test_close_the_loop(emu_lib):
    where_text_cases.close_the_loop(emu_lib)


def test_capacity(emu_lib):
    where_text_cases.capacity(emu_lib)


def test_errors(emu_lib):
    where_text_cases.errors(emu_lib)


def test_damaged_member(emu_lib):
    where_text_cases.damaged(emu_lib)
