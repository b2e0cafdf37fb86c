"""The search through the CPU emulator (a device pointer is a host pointer there): the shared bodies of
tests/find_cases.py, every count, position and line compared with what bytes.find and numpy give on zlib's inflate of the
same members."""
import find_cases


def test_hits_planted(emu_lib):
    find_cases.hits_planted(emu_lib)


def test_hits_small_members(emu_lib):
    find_cases.hits_small_members(emu_lib)


def test_hits_newline(emu_lib, oracle):
    find_cases.hits_newline(emu_lib, oracle)


def test_hits_special_bytes(emu_lib):
    find_cases.hits_special_bytes(emu_lib)


def test_hits_overlaps(emu_lib):
    find_cases.hits_overlaps(emu_lib)


def test_hits_edges(emu_lib):
    find_cases.hits_edges(emu_lib)


def test_batches_tiny_members(emu_lib):
    find_cases.batches_tiny_members(emu_lib)


def test_batches_every_split(emu_lib):
    find_cases.batches_every_split(emu_lib)


def test_lines(emu_lib):
    find_cases.lines(emu_lib)


def test_lines_close_the_loop(emu_lib):
    find_cases.lines_close_the_loop(emu_lib)


def test_capacity(emu_lib):
    find_cases.capacity(emu_lib)


def test_errors(emu_lib):
    find_cases.errors(emu_lib)


def test_damaged_member(emu_lib):
    find_cases.damaged(emu_lib)
