"""The selection of lines by their numbers through the CPU emulator (a device pointer is a host pointer there): the
shared bodies of tests/where_cases.py, every run and count compared with a Python model of the rules on zlib's inflate of
the same members."""
import where_cases


def test_operators(emu_lib):
    where_cases.operators(emu_lib)


def test_most_terms(emu_lib):
    where_cases.most_terms(emu_lib)


def test_edges_of_the_walk(emu_lib):
    where_cases.edges(emu_lib)


def test_runs(emu_lib):
    where_cases.runs(emu_lib)


def test_scan_step(emu_lib):
    where_cases.scan_step(emu_lib, both_forms=False)


def test_capacity(emu_lib):
    where_cases.capacity(emu_lib)


def test_errors(emu_lib):
    where_cases.errors(emu_lib)


def test_damaged_member(emu_lib):
    where_cases.damaged(emu_lib)


def test_close_the_loop(emu_lib):
    where_cases.close_the_loop(emu_lib)
